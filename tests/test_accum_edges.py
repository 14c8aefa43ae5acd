"""The sparse accumulation (csrc/msr_accumulate.hpp: accumulate_tile, accumulate_tile_light) and the selection behind it
on planted corpora aimed at their branch edges (tests/accum_ref.py): chunk and segment geometry, the 256-entry rounds,
the light / general switch, the dense head's pair pipeline, ragged last tiles, and scores in [2^31, 2^32).

Every case asserts, before it searches, the census facts it is named after; tests/test_accum_ref.py proves on the CPU
that the lists cover the whole edge list and that the C oracle used here equals a plain numpy D @ q on these corpora.
Comparison is exact through helpers.assert_same_results: ordinals, u32 scores, hit counts, f32 bits, padding."""
import numpy as np
import pytest

from tests import accum_ref as ar
from tests import helpers

pytestmark = pytest.mark.gpu

E_OVERFLOW, E_RANGE = -7, -8


@pytest.fixture(scope="module")
def m(built):
    import mllm_sparse_retrieval_amd as m

    return m


def _assert_facts(path, cases, k, light):
    cen = ar.census(path, ar.csr([c.entries for c in cases]), k)
    assert cen["batch"]["light"] == light, cen["batch"]
    for qi, c in enumerate(cases):
        assert cen["queries"][qi]["error"] is None, c.edges
        for fact in c.facts:
            ar.check_fact(cen, qi, fact)
    return cen


def _identical(a, b, rows):
    for x, y in zip(a[:3], b[:3]):
        assert (np.ascontiguousarray(x[:rows]).view(np.uint32) == np.ascontiguousarray(y[:rows]).view(np.uint32)).all()
    assert (a[3][:rows] == b[3][:rows]).all()


def _search_all(ix, oix, batches, ks, drop=True):
    """Every batch through search_csr and through a resident batch at every k, against the oracle -> {(batch, k): result}."""
    out = {}
    for bi, queries in enumerate(batches):
        b = ix.batch(*queries, max(ks), drop_df_eq_n=drop)
        try:
            for k in ks:
                want = oix.search(*queries, k, drop_df_eq_n=drop, threads=8)
                got = ix.search_csr(*queries, k, drop_df_eq_n=drop)
                helpers.assert_same_results(got, want, k)
                b.search(k)
                helpers.assert_same_results(b.fetch(), want, k)
                out[bi, k] = got
        finally:
            b.close()
    return out


# ------------------------------------------------------------------------------------------ accumulation geometry
@pytest.mark.parametrize("n_dense,last_label", ar.GEOMETRY_VARIANTS, ids=[f"dense{a}-last_{b.replace(' ', '_')}"
                                                                           for a, b in ar.GEOMETRY_VARIANTS])
@pytest.mark.parametrize("tile_docs", ar.TILE_SIZES)
def test_geometry(m, tmp_path, tile_docs, n_dense, last_label):
    p = ar.geometry_corpus(tile_docs, last_label, n_dense)
    path = ar.build(m, tmp_path / "g.idx", p, n_dense, ar.DENSE_DENSITY)
    light, general = ar.geometry_cases(p)
    named = {e for c in light + general for e in c.edges}
    assert not [e for e in ar.geometry_required(tile_docs, n_dense, last_label) if e not in named]
    # k = 10: the 512-key instances (light where the tile size has one); k = 1000: the 1024-key instance
    _assert_facts(path, light, 10, tile_docs in ar.LIGHT_TILES)
    _assert_facts(path, light + general, 10, False)
    _assert_facts(path, light + general, 1000, False)
    oix, _ = helpers.taat_oracle(p["docs"], p["n_terms"], p["ids"])
    lq, gq = ar.csr([c.entries for c in light]), ar.csr([c.entries for c in light + general])
    mixed = ar.mixed_batch(light, general)
    cm = _assert_facts(path, mixed, 10, False)
    assert [q["n_sparse"] > ar.LIGHT_MAX for q in cm["queries"]] == [False] * len(light) + [True]
    assert cm["queries"][-1]["n_sparse"] == 65
    mq = ar.csr([c.entries for c in mixed])
    with m.SparseIndex(path, device=0) as ix:
        assert ix.n_dense == n_dense + n_dense % 2 and ix.n_tiles == 2
        res = _search_all(ix, oix, [lq, gq, mq], (10, 1000))
    # a batch that is light except for ONE 65-entry query (and the batch with every general case): query by query what
    # the all-light batch returns
    for k in (10, 1000):
        _identical(res[0, k], res[2, k], len(light))
        _identical(res[0, k], res[1, k], len(light))


@pytest.mark.parametrize("n_dense", ar.OTHER_USERS["n_dense"])
def test_other_users_of_the_accumulation(m, tmp_path, n_dense):
    """The same planted index (three tiles) through doc-range shards + merge_lists (non-zero vec_base), term-range
    shard handles (term_base columns, dump mode) and the emulated term-shard protocol: the same oracle results."""
    ou = ar.OTHER_USERS
    p = ar.geometry_corpus(ou["tile_docs"], n_dense=n_dense, n_full=ou["n_full"])
    path = ar.build(m, tmp_path / "g.idx", p, n_dense, ar.DENSE_DENSITY)
    light, general = ar.geometry_cases(p)
    cases = light + general
    _assert_facts(path, cases, 10, False)
    queries = ar.csr([c.entries for c in cases])
    oix, _ = helpers.taat_oracle(p["docs"], p["n_terms"], p["ids"])
    n_sh = ou["doc_shards"]
    with m.SparseIndex(path, device=0) as ix:
        assert ix.n_tiles == ou["n_full"] + 1 == n_sh
        for k in ou["ks"]:
            want = oix.search(*queries, k, threads=8)
            lists = []
            for s in range(n_sh):
                with m.SparseIndex(path, device=0, shard=s, n_shards=n_sh) as sh:
                    assert sh.shard_ntiles == 1 and sh.shard_tile0 == s
                    lists.append(sh.search_csr(*queries, k))
            merged = ix.merge_lists(np.stack([l[0] for l in lists]), np.stack([l[2] for l in lists]),
                                    np.stack([l[3] for l in lists]), k)
            helpers.assert_same_results(merged, want, k)
            for G in ou["term_shards"]:
                helpers.assert_same_results(ix.search_termshard_emulated(*queries, k, G), want, k)
                shards = [m.SparseIndex(path, device=0, term_shard=(g, G)) for g in range(G)]
                try:
                    assert shards[1].term_lo > 0
                    helpers.assert_same_results(m.search_termshard_emulated_handles(shards, *queries, k), want, k)
                finally:
                    for sh in shards:
                        sh.close()


# --------------------------------------------------------------------------------- the top of the score range
def _top_scores(D, name):
    s = np.zeros(D.shape[0], dtype=np.int64)
    for t, w in ar.TOP_QUERIES[name]:
        s += D[:, t] * w
    return s


@pytest.mark.parametrize("variant,dmax,density", ar.top_variants(), ids=[v[0] for v in ar.top_variants()])
@pytest.mark.parametrize("tile_docs", ar.TILE_SIZES)
def test_top_of_the_score_range(m, tmp_path, tile_docs, variant, dmax, density):
    p = ar.top_corpus(tile_docs)
    path = ar.build(m, tmp_path / "t.idx", p, dmax, density)
    names = list(ar.TOP_QUERIES)
    lq = ar.csr([ar.TOP_QUERIES[n] for n in names])
    gq = ar.csr([ar.TOP_QUERIES[n] for n in names] + [ar.TOP_GENERAL_EXTRA])
    ixf = helpers.read_index_file(path)
    D = helpers.index_file_to_dense(ixf)
    assert [int(t) for t in ixf["dense_terms"]] == ([0, ar.NO_TERM] if variant == "dense" else [])
    # census: bounds fit, the batches are light / general, bit 31 is set in every hit of the plateau queries, and the
    # plateau forces the selection the case is here for
    for k in ar.TOP_KS:
        cl, cg = ar.census(ixf, lq, k), ar.census(ixf, gq, k)
        assert all(q["error"] is None and q["bound"] <= 0xFFFFFFFF for q in cg["queries"])
        assert cl["batch"]["light"] == (tile_docs in ar.LIGHT_TILES and k <= 512) and not cg["batch"]["light"]
        for n in ("plateau top", "two scores", "65535 x 65535 tied"):
            s = _top_scores(D, n)
            assert s[s > 0].min() >= 2**31
            assert ar.select_path(s[:tile_docs], tile_docs, k) == ("hist" if tile_docs <= 8192 and k > 512 else "radix")
        if k >= 256:    # 100 distinct docs above the plateau: it straddles the k-th place from there on
            s = _top_scores(D, "plateau mid")
            assert ar.select_path(s[:tile_docs], tile_docs, k) == ("hist" if tile_docs <= 8192 and k > 512 else "radix")
    assert _top_scores(D, "peak 0xFFFFFFFF").max() == 0xFFFFFFFF and _top_scores(D, "u24 weight 0xFFFFFF").max() == 255 * 0xFFFFFF
    oix, _ = helpers.taat_oracle(p["docs"], p["n_terms"], p["ids"])
    with m.SparseIndex(path, device=0) as ix:
        res = _search_all(ix, oix, [lq, gq], ar.TOP_KS)
    for k in ar.TOP_KS:
        _identical(res[0, k], res[1, k], len(names))
    o, f, u, n = res[0, 1024]
    i = names.index("peak 0xFFFFFFFF")
    assert n[i] == 2 and list(u[i, :2]) == [0xFFFFFFFF, 0xFFFEFFFE] and list(o[i, :2]) == [7, tile_docs + 3]
    assert list(f[i, :2]) == [np.float32(2**32), np.float32(0xFFFEFFFE)]   # both round up: (float)u32, nearest even
    assert u[names.index("65535 x 65535 tied"), 0] == 65535 * 65535 and n[names.index("distinct")] == 1024


@pytest.mark.parametrize("variant,dmax,density", ar.top_variants(), ids=[v[0] for v in ar.top_variants()])
def test_refusals_at_their_exact_limits(m, tmp_path, variant, dmax, density):
    from mllm_sparse_retrieval_amd._cabi import MsrError

    p = ar.top_corpus(4096)
    path = ar.build(m, tmp_path / "t.idx", p, dmax, density)
    ixf = helpers.read_index_file(path)
    oix, _ = helpers.taat_oracle(p["docs"], p["n_terms"], p["ids"])
    code = {"RANGE": E_RANGE, "OVERFLOW": E_OVERFLOW}
    cases = ar.TOP_REFUSALS + ([ar.TOP_REFUSAL_DENSE] if variant == "dense" else [])
    with m.SparseIndex(path, device=0) as ix:
        for label, bad, err, ok in cases:
            assert ar.census(ixf, ar.csr([bad]), 10)["queries"][0]["error"] == err, label
            assert ar.census(ixf, ar.csr([ok]), 10)["queries"][0]["error"] is None, label
            with pytest.raises(MsrError) as e:
                ix.search_csr(*ar.csr([bad]), 10)
            assert e.value.code == code[err], (label, str(e.value))
            with pytest.raises(MsrError) as e:
                ix.batch(*ar.csr([bad]), 10)
            assert e.value.code == code[err], (label, str(e.value))
            if err == "OVERFLOW":   # (the oracle has the bound too; the weight limits are the kernels' own)
                with pytest.raises(OverflowError):
                    oix.search(*ar.csr([bad]), 10)
            helpers.assert_same_results(ix.search_csr(*ar.csr([ok]), 10), oix.search(*ar.csr([ok]), 10), 10)


# ------------------------------------------------------------------------- the fused hybrid kernels at the top
@pytest.mark.parametrize("shape,tile_docs,n_docs,dmax", ar.HYBRID_SHAPES, ids=["single", "multi"])
def test_hybrid_union_at_the_top_of_the_range(m, tmp_path, shape, tile_docs, n_docs, dmax):
    """msr_hybrid_search_union on an f32 handle with sparse scores in [2^31, 2^32): the exact u32 score of every sparse
    member, the sparse depth list, float32 of the best and depth-th exact score and the fused order are those of the
    oracle pipeline (helpers.check_union with the project's UNION_TOL and UNION_TIE). Sparse scores collapse to f32
    before fusion in the kernel and the oracle alike, so equal fused scores are true ties. Queries 3-5 are the tight
    cluster: more than 512 docs within 255 of each other, below the f32 spacing of 256, so the value-linear histogram
    of hybrid_tiles holds them in one bin and the exact path behind kHistCand decides the depth-th place."""
    from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_search_union, row_to_ordinal

    depth, alpha, h = ar.HYBRID_DEPTH, 0.5, 64
    p = ar.hybrid_corpus(tile_docs, n_docs)
    path = ar.build(m, tmp_path / "h.idx", p, dmax, 0.9)   # dmax = 1: the carrier alone in the dense head
    qp, qt, qw = ar.csr(p["queries"])
    nq = len(qp) - 1
    ixf = helpers.read_index_file(path)
    D = helpers.index_file_to_dense(ixf)
    assert ixf["n_tiles"] == (1 if shape == "single tile" else 3) and ixf["n_dense"] == 2 * dmax
    cen = ar.census(ixf, (qp, qt, qw), depth)
    assert all(q["error"] is None and q["pairs"] == dmax and q["n_sparse"] == 2 - dmax for q in cen["queries"])
    ar.assert_hybrid_corpus(p, D, depth)
    rng = np.random.default_rng(9)
    pm, q = rng.standard_normal((n_docs, h)).astype(np.float32), rng.standard_normal((nq, h)).astype(np.float32)
    qids = [f"q{i}" for i in range(nq)]
    with m.SparseIndex(path, device=0) as ix:
        dix = DenseIndex(pm, precision="f32")
        try:
            r2o = row_to_ordinal(ix, p["ids"])
            assert (r2o == np.arange(n_docs)).all()
            res = hybrid_search_union(ix, dix, qp, qt, qw, q, depth, alpha, r2o, None)
            d_sc, d_rows, s_all = helpers.union_dense_lists(q, pm, depth, "f32", r2o)
            sample = np.arange(nq)
            o_sparse, o_dense, exact, sq = helpers.union_oracle_runs(p["docs"], p["n_terms"], p["ids"], qp, qt, qw, sample,
                                                                     depth, False, qids, d_sc, d_rows)
            row_of = {d: r for r, d in enumerate(p["ids"])}
            helpers.check_union(res, sample, sq, o_sparse, o_dense, exact, alpha, depth, ix,
                                lambda j, doc: s_all[j, row_of[doc]])
            # stated once more on the raw arrays: exact scores where the sparse bit is set, range = f32 of best / depth-th
            ords, fs, cnt, src, su, de, rg, _ = res
            for i in range(nq):
                s = sum(D[:, t] * w for t, w in p["queries"][i])
                live = np.arange(2 * depth) < cnt[i]
                sp = live & ((src[i] & 2) != 0)
                order = np.lexsort((np.arange(n_docs), -s))[:depth]
                assert sp.sum() == depth and set(ords[i][sp].tolist()) == set(order.tolist())
                assert (su[i][sp].astype(np.int64) == s[ords[i][sp]]).all()
                want = np.array([s[order[0]], s[order[-1]]]).astype(np.float32)
                assert (rg[i, 2:4].view(np.uint32) == want.view(np.uint32)).all()
        finally:
            dix.close()
