"""CPU checks of tests/accum_ref.py: the planted corpora are what the built index file holds, the census of every GPU
case list (tests/test_accum_edges.py) covers the full edge list by name, the C oracle equals the plain numpy reference
on every planted corpus (the top-of-range ones included), and the instance table restated in the census is the one in
the source text of with_tile_shape and launch_score. None of this needs a GPU: the index builder and the oracle are
host code."""
import os
import re

import numpy as np
import pytest

from tests import accum_ref as ar
from tests import helpers

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mllm_sparse_retrieval_amd", "csrc")


@pytest.fixture(scope="module")
def m(built):
    import mllm_sparse_retrieval_amd as m

    return m


def _src(name):
    with open(os.path.join(CSRC, name), encoding="utf-8") as f:
        return f.read()


def test_instance_table_is_the_one_of_launch_score():
    dev, internal = _src("msr_device.hip"), _src("msr_device_internal.hpp")
    # ONE table (with_tile_shape): every launcher of the two units goes through its switch
    rows = re.findall(r"case (\d+): f\(TileShape<(\d+), (\d+), (\d+), \d+, \d+>\{\}\); return true;", internal)
    assert {int(t): (int(n), int(u)) for t, _, n, u in rows} == ar.INSTANCES and all(t == t2 for t, t2, _, _ in rows)
    assert "static constexpr bool light = DOCS == 4096 || DOCS == 8192;" in internal and ar.LIGHT_TILES == (4096, 8192)
    every = "".join(_src(f) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp")))
    for t in ar.INSTANCES:
        assert every.count(f"case {t}:") == 1, t
    rule = dev[dev.index("static int launch_score("):dev.index("int launch_select(")]
    assert "constexpr uint32_t T = S::docs, N = S::threads, UU = S::loads, W = S::waves, WR = S::waves_rest;" in rule
    # dump / light with the 512-key buffer / k <= 512 / the 1024-key buffer, in this order
    assert re.search(r"if \(dump\)\s*hipLaunchKernelGGL\(\(score_tiles<T, N, UU, WR, 512, 1>\), grid, dim3\(N\), 0, st, a\);\s*"
                     r"else if \(a\.k <= 512 && a\.light && S::light\)\s*"
                     r"hipLaunchKernelGGL\(\(score_tiles<T, N, UU, W, 512, 0, S::light>\), grid, dim3\(N\), 0, st, a\);\s*"
                     r"else if \(a\.k <= 512\)\s*hipLaunchKernelGGL\(\(score_tiles<T, N, UU, W, 512>\), grid, dim3\(N\), 0, st, a\);\s*"
                     r"else\s*hipLaunchKernelGGL\(\(score_tiles<T, N, UU, WR, 1024>\), grid, dim3\(N\), 0, st, a\);", rule)
    assert "sa.light = b->max_sparse_terms <= 64 ? 1u : 0u;" in dev and ar.LIGHT_MAX == 64
    assert re.search(rf"constexpr int kQtBlock = {ar.KQT_BLOCK};", internal)
    assert re.search(rf"constexpr int kChunkVecs = {ar.CHUNK_VECS};", internal)
    assert f"constexpr int UL = {ar.UL};" in _src("msr_accumulate.hpp")
    assert "if (TILE_DOCS <= 8192 && CAND >= 2 * kHistCand && n_cand > CAND)" in _src("msr_select.hpp")
    assert "constexpr int kHistCand = 512;" in _src("msr_hist_select.hpp")


def _both_references(path, p, queries, ks, drop=True):
    """oracle == numpy reference on the built file at every k of `ks`."""
    ix = helpers.read_index_file(path)
    D = helpers.index_file_to_dense(ix)
    oix, _ = helpers.taat_oracle(p["docs"], p["n_terms"], p["ids"])
    S = ar.numpy_scores(ix, D, queries, drop)
    for k in ks:
        want, ref = oix.search(*queries, k, drop_df_eq_n=drop, threads=8), ar.rank(S, k)
        assert (want[2] == ref[2]).all()
        mask = np.arange(k)[None, :] < ref[2][:, None]
        assert (want[0][mask] == ref[0][mask]).all() and (want[1][mask] == ref[1][mask]).all()
    return ix, D


@pytest.mark.parametrize("tile_docs", ar.TILE_SIZES)
def test_planted_counts_are_what_the_file_holds(m, tmp_path, tile_docs):
    for n_dense in (0, 32, 5):
        p = ar.geometry_corpus(tile_docs, n_dense=n_dense, n_full=2 if tile_docs == 4096 else 1)
        ix = helpers.read_index_file(ar.build(m, tmp_path / "g.idx", p, n_dense, ar.DENSE_DENSITY))
        r = p["roles"]
        assert ix["n_tiles"] == len(p["sizes"]) and ix["n_docs"] == p["n_docs"] and ix["docs"] == p["ids"]
        assert ix["n_dense"] == n_dense + n_dense % 2
        assert [int(t) for t in ix["dense_terms"][:n_dense]] == r["dense"]     # slot s holds planted dense term s
        sparse = np.setdiff1d(np.arange(p["n_terms"]), r["dense"])
        vecs = np.diff(ix["seg_ptr"].astype(np.int64), axis=1)
        assert (vecs[:, sparse] == (p["per"][:, sparse] + 3) // 4).all()     # ceil(m / 4) vecs per (tile, term)
        assert (vecs[:, r["dense"]] == 0).all()
        assert (ar.segment_postings(ix)[:, sparse] == p["per"][:, sparse]).all()
        for s, t in enumerate(r["dense"]):                                    # dense rows hold the planted counts
            row = (ix["dense"][:, s // 2, :] >> (16 * (s & 1))) & 0xFFFF
            assert ((row != 0).sum(axis=1) == p["per"][:, t]).all()
        assert (ix["df"] == p["per"].sum(axis=0)).all()


def _geometry_census(m, tmp_path, tile_docs, n_dense, last_label):
    p = ar.geometry_corpus(tile_docs, last_label, n_dense)
    path = ar.build(m, tmp_path / "g.idx", p, n_dense, ar.DENSE_DENSITY)
    light, general = ar.geometry_cases(p)
    edges = set()
    for cases, k in ((light, 10), (light + general, 10), (light + general, 1000)):
        cen = ar.census(path, ar.csr([c.entries for c in cases]), k)
        assert cen["batch"]["light_batch"] == (cases is light)
        assert cen["batch"]["light"] == (cases is light and tile_docs in ar.LIGHT_TILES)
        for qi, c in enumerate(cases):
            assert cen["queries"][qi]["error"] is None
            for fact in c.facts:
                ar.check_fact(cen, qi, fact)
            edges.update(c.edges)
    return p, path, light, general, edges


@pytest.mark.parametrize("tile_docs", ar.TILE_SIZES)
def test_geometry_cases_cover_every_edge(m, tmp_path, tile_docs):
    for n_dense, last_label in ar.GEOMETRY_VARIANTS:
        p, path, light, general, edges = _geometry_census(m, tmp_path, tile_docs, n_dense, last_label)
        for name in ar.geometry_required(tile_docs, n_dense, last_label):   # one assertion per edge
            assert name in edges, (tile_docs, n_dense, last_label, name)
        assert max(len(c.entries) for c in light) <= ar.LIGHT_MAX
        _both_references(path, p, ar.csr([c.entries for c in light + general]), (10, 1000))   # the two references agree
        # the batch that is light except for one 65-entry query
        mixed = ar.mixed_batch(light, general)
        cen = ar.census(path, ar.csr([c.entries for c in mixed]), 10)
        assert [q["n_sparse"] for q in cen["queries"]][-1] == 65 and not cen["batch"]["light"], "mixed batch"
        assert max(q["n_sparse"] for q in cen["queries"][:-1]) <= ar.LIGHT_MAX, "mixed batch: the rest is light"
        if n_dense and last_label == "1":   # the one-doc last tile holds a dense-head posting
            assert (helpers.read_index_file(path)["dense"][-1, 0, :] & 0xFFFF).any()
    # the variants themselves: every last-tile shape with and without a dense head, an odd head, all 16 pairs
    assert {lab for _, lab in ar.GEOMETRY_VARIANTS} == set(ar.LAST_TILES)
    assert all({(0, lab), (32, lab)} <= set(ar.GEOMETRY_VARIANTS) for lab in ar.LAST_TILES)
    assert any(nd % 2 for nd, _ in ar.GEOMETRY_VARIANTS)


def top_paths(ix, D, p, name, k):
    """(scores of the k-th hit, selection path in tile 0) of a top-of-range query, from the numpy scores."""
    s = np.zeros(ix["n_docs"], dtype=np.int64)
    for t, w in ar.TOP_QUERIES[name]:
        s += D[:, t] * w
    return s, ar.select_path(s[:p["tile_docs"]], p["tile_docs"], k)


@pytest.mark.parametrize("tile_docs", ar.TILE_SIZES)
def test_top_of_range_cases_cover_every_edge(m, tmp_path, tile_docs):
    p = ar.top_corpus(tile_docs)
    names = list(ar.TOP_QUERIES)
    for variant, dmax, dens in ar.top_variants():
        path = ar.build(m, tmp_path / "t.idx", p, dmax, dens)
        queries = ar.csr([ar.TOP_QUERIES[n] for n in names] + [ar.TOP_GENERAL_EXTRA])
        ix, D = _both_references(path, p, queries, (1, 1024))      # the oracle raises on overflow: every bound fits
        assert [int(t) for t in ix["dense_terms"]] == ([0, ar.NO_TERM] if variant == "dense" else [])
        cen = ar.census(ix, queries, 1024)
        assert all(q["error"] is None and q["bound"] <= 0xFFFFFFFF for q in cen["queries"])
        assert cen["queries"][names.index("peak 0xFFFFFFFF")]["bound"] == 0xFFFFFFFF
        assert not cen["batch"]["light_batch"] and ar.census(ix, ar.csr([ar.TOP_QUERIES[n] for n in names]), 1)["batch"]["light_batch"]
        # score distributions
        s = {n: top_paths(ix, D, p, n, 1)[0] for n in names}
        hits = s["distinct"][s["distinct"] > 0]
        assert len(np.unique(hits)) == len(hits) == p["n_docs"] - 1 and hits.min() >= 2**31, "all distinct"
        top = s["plateau top"]
        assert (top == top.max()).sum() == ar.PLATEAU > 1024 and top.max() >= 2**31, "plateau at the top"
        mid = s["plateau mid"]
        tied = np.bincount(np.unique(mid, return_inverse=True)[1]).max()
        assert tied == ar.PLATEAU and (mid > np.median(mid[p["plateau"]])).sum() == 100, "plateau below 100 distinct docs"
        assert sorted(np.unique(s["two scores"][s["two scores"] > 0])) == [65535 * ar.W_CARRIER, 65535 * ar.W_CARRIER + 7]
        assert sorted(s["peak 0xFFFFFFFF"][s["peak 0xFFFFFFFF"] > 0]) == [0xFFFEFFFE, 0xFFFFFFFF], "single hit at the top"
        assert s["u24 weight 0xFFFFFF"].max() == 255 * 0xFFFFFF and ix["maxw"][5] == 255
        assert s["65535 x 65535 tied"].max() == 65535 * 65535 and (s["65535 x 65535"] >= 65535 * 65535).sum() == p["n_docs"] - 1
        # selections met with bit 31 set in every candidate: per k the path of tile 0, named
        met = set()
        for k in ar.TOP_KS:
            for n in ("plateau top", "plateau mid", "two scores", "distinct", "65535 x 65535 tied"):
                sc, path_k = top_paths(ix, D, p, n, k)
                assert sc[sc > 0].min() >= 2**31
                met.add((path_k, 512 if k <= 512 else 1024, ar.switch_of(tile_docs, k)))
            assert top_paths(ix, D, p, "plateau top", k)[1] == ("hist" if tile_docs <= 8192 and k > 512 else "radix")
        nt = ar.INSTANCES[tile_docs][0]
        big = "hist" if tile_docs <= 8192 else "radix"
        for edge in [("radix", 512, "k<=64"), ("radix", 512, "k<=NT"), (big, 1024, "k<=NT" if nt == 1024 else "k>NT")] + \
                    ([("radix", 512, "k>NT")] if nt < 512 else []):
            assert edge in met, (tile_docs, variant, edge)
        # refusals at their exact limits, and their accepted neighbours
        for label, bad, err, ok in ar.TOP_REFUSALS + ([ar.TOP_REFUSAL_DENSE] if variant == "dense" else []):
            cb, co = ar.census(ix, ar.csr([bad]), 1), ar.census(ix, ar.csr([ok]), 1)
            assert cb["queries"][0]["error"] == err and co["queries"][0]["error"] is None, label
        assert ar.census(ix, ar.csr([[(4, 65537), (6, 1)]]), 1)["queries"][0]["bound"] == 2**32
        with pytest.raises(OverflowError):
            helpers.taat_oracle(p["docs"], p["n_terms"], p["ids"])[0].search(*ar.csr([[(4, 65537), (6, 1)]]), 1)
    assert set(ar.TOP_KS) == {1, 64, 65, 256, 257, 512, 513, 1000, 1024}


def test_census_restates_the_host_normalisation(m, tmp_path):
    # OOV and non-positive weights vanish, df == N terms go under the flag only, dense-head terms leave the sparse
    # list and add up per slot, repeated sparse terms stay separate entries
    p = ar.geometry_corpus(4096, n_dense=5)
    every = p["n_terms"]
    p2 = ar.plant(4096, p["n_docs"], every + 2, {**{t: list(p["per"][:, t]) for t in range(every)},
                                                  every: list(p["sizes"])}, seed=0)
    path = ar.build(m, tmp_path / "n.idx", p2, 5, ar.DENSE_DENSITY)   # term `every`: df == N; every + 1: df == 0
    ix = helpers.read_index_file(path)
    d, f = p["roles"]["dense"], p["roles"]["fill"]
    assert ix["df"][every] == ix["n_docs"] and ix["df"][every + 1] == 0
    # (df == N outranks the planted dense terms: it takes slot 0 and pushes the fifth planted term out of the head)
    assert [int(t) for t in ix["dense_terms"]] == [every] + d[:4] + [ar.NO_TERM]
    ents = [(-1, 5), (f[0], 0), (f[0], -3), (f[1], 2), (every, 9), (every + 1, 4), (d[0], 7), (f[1], 3), (d[0], 8), (d[4], 2)]
    q = ar.census(ix, ar.csr([ents]), 10)["queries"][0]
    assert q["n_sparse"] == 3 and q["dsum"] == [0, 15, 0, 0, 0, 0] and q["halves"] == {0: "hi"}
    q = ar.census(ix, ar.csr([ents]), 10, drop_df_eq_n=False)["queries"][0]
    assert q["n_sparse"] == 3 and q["dsum"] == [9, 15, 0, 0, 0, 0] and q["halves"] == {0: "both"}
    assert ar.census(ix, ar.csr([[(every + 2, 1)]]), 10)["queries"][0]["error"] == "RANGE"



@pytest.mark.parametrize("n_dense", ar.OTHER_USERS["n_dense"])
def test_other_users_corpora(m, tmp_path, n_dense):
    """The three-tile corpora of the doc-shard / term-shard cases: the edges they are there for, and both references."""
    ou = ar.OTHER_USERS
    assert ou["term_shards"] == (2, 3) and ou["n_dense"] == (0, 32), "term-range shards with G = 2 and 3, with and without a dense head"
    p = ar.geometry_corpus(ou["tile_docs"], n_dense=n_dense, n_full=ou["n_full"])
    path = ar.build(m, tmp_path / "g.idx", p, n_dense, ar.DENSE_DENSITY)
    ix = helpers.read_index_file(path)
    assert ix["n_tiles"] == ou["doc_shards"] == 3, "doc-range shards: one tile each"
    assert (ix["seg_ptr"][1:, 0] > 0).all(), "doc-range shards: non-zero vec_base in the later shards"
    assert ix["n_dense"] == n_dense
    light, general = ar.geometry_cases(p)
    cen = ar.census(ix, ar.csr([c.entries for c in light + general]), 10)
    for qi, c in enumerate(light + general):
        for fact in c.facts:
            ar.check_fact(cen, qi, fact)
    # term-range shards: each of the G ranges owns terms the queries hold (bounds are the library's; thirds suffice here)
    held = {t for c in light + general for t, _ in c.entries}
    assert all(any(lo <= t < lo + p["n_terms"] // 3 for t in held) for lo in (0, p["n_terms"] // 3, 2 * (p["n_terms"] // 3)))
    _both_references(path, p, ar.csr([c.entries for c in light + general]), ou["ks"])


@pytest.mark.parametrize("shape,tile_docs,n_docs,dmax", ar.HYBRID_SHAPES, ids=["single", "multi"])
def test_hybrid_corpora(m, tmp_path, shape, tile_docs, n_docs, dmax):
    """The two hybrid shapes: single and multi-tile, top-of-range depth lists, the tight cluster, both references."""
    assert [s[0] for s in ar.HYBRID_SHAPES] == ["single tile", "multi-tile"]
    p = ar.hybrid_corpus(tile_docs, n_docs)
    path = ar.build(m, tmp_path / "h.idx", p, dmax, 0.9)
    queries = ar.csr(p["queries"])
    ix, D = _both_references(path, p, queries, (1, ar.HYBRID_DEPTH))
    assert (ix["n_tiles"] == 1) == (shape == "single tile") and ix["n_tiles"] in (1, 3)
    assert ix["tile_docs"] in ar.LIGHT_TILES     # the tile sizes the fused hybrid kernels have
    cen = ar.census(ix, queries, ar.HYBRID_DEPTH)
    assert all(q["error"] is None and q["pairs"] == dmax and q["n_sparse"] == 2 - dmax for q in cen["queries"])
    assert len(p["tight"]) == 3 and len(p["queries"]) == 6
    ar.assert_hybrid_corpus(p, D)   # depth lists in [2^31, 2^32); > 512 docs within 255; one and two f32 values
