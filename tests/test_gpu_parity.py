"""GPU parity tests proper: the HIP path, called through the C-ABI, against the oracle on the same seeded inputs.

Bar: bit-exact doc ordinals and exact integer scores; f32 scores within 1e-5 (north_star) — in fact equal.
"""
import os

import numpy as np
import pytest

from tests import helpers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m(built):
    import mllm_sparse_retrieval_amd as m

    return m


def _case(m, tmp_path, n_docs, doc_nnz, nq, q_nnz, n_terms, seed, tile_docs, ks, doc_ids=None, dense_max=16,
          dense_density=0.4):
    docs, (qp, qt, qw) = helpers.synth(n_docs, doc_nnz, nq, q_nnz, n_terms, seed)
    m.set_build_option("dense_max_terms", dense_max)
    m.set_build_option("dense_min_density", dense_density)
    try:
        path = m.build_index_from_csr(str(tmp_path / "c.idx"), *docs, n_terms, doc_ids=doc_ids, tile_docs=tile_docs)
    finally:
        m.set_build_option("dense_max_terms", 16)
        m.set_build_option("dense_min_density", 0.4)
    oix, _ = helpers.taat_oracle(docs, n_terms, doc_ids)
    with m.SparseIndex(path, device=0) as ix:
        for k in ks:
            got = ix.search_csr(qp, qt, qw, k)
            want = oix.search(qp, qt, qw, k, threads=8)
            helpers.assert_same_results(got, want, k)


@pytest.mark.parametrize("tile_docs", [4096, 8192, 16384, 32768])
@pytest.mark.parametrize("dense_max,density", [(16, 0.4), (0, 0.4), (32, 0.02), (5, 0.1)])
def test_single_and_multi_tile(m, tmp_path, tile_docs, dense_max, density):
    # 20k docs: 5 / 3 / 2 / 1 tiles, last tile ragged; with / without / with a large / with an odd-sized dense head
    _case(m, tmp_path, 20000, 64, 200, 40, 5000, seed=21, tile_docs=tile_docs, ks=[1, 10, 100], dense_max=dense_max,
          dense_density=density)


def test_flickr_shape_c2(m, tmp_path):
    # BASELINE config 2: 1 000 docs x 128 nnz, 5 000 queries, V = 32 064, top-10
    _case(m, tmp_path, 1000, 128, 5000, 12, 32064, seed=1, tile_docs=0, ks=[10])


def test_flickr_headline_full_shape(m, tmp_path):
    # The bench's headline workload at its real size (BASELINE configs 1/2 on the whole Flickr30K: 31 014 image docs x
    # 128 nnz, ALL 155 070 caption queries of 8-15 terms, V = 32 064, top-10, default tile): every query against the C
    # oracle, through the resident batch the bench times and through one msr_search_csr call (threaded normalisation)
    from mllm_sparse_retrieval_amd import workloads

    wl = workloads.flickr30k_t2i(threads=8)
    qp, qt, qw = wl.queries
    assert len(qp) - 1 == 155070
    path = m.build_index_from_csr(str(tmp_path / "f.idx"), *wl.docs, wl.n_terms, threads=8, tile_docs=0)
    oix, _ = helpers.taat_oracle(wl.docs, wl.n_terms)
    want = oix.search(qp, qt, qw, 10, threads=16)
    with m.SparseIndex(path, device=0) as ix:
        assert ix.n_tiles == 4 and ix.tile_docs == 8192
        batch = ix.batch(qp, qt, qw, 10)
        batch.search(10)
        batch.search(10)                                   # (a second pass over the resident batch: same result)
        helpers.assert_same_results(batch.fetch(), want, 10)
        helpers.assert_same_results(ix.search_csr(qp, qt, qw, 10), want, 10)
        got = batch.fetch()
        # Recall@1/5/10 as the bench prints it (qrels: caption j <-> image j // 5): the planted captions make it a
        # meaningful number — not 0, not trivially 1 at k = 1
        doc_int = np.array([int(ix.docid(o)) for o in range(ix.n_docs)], dtype=np.int64)
    ranked = np.where(np.arange(10)[None, :] < got[3][:, None], doc_int[np.minimum(got[0], 31013)], -1)
    target = (np.arange(155070) // 5)[:, None]
    r1, r10 = [(ranked[:, :k] == target).any(axis=1).mean() for k in (1, 10)]
    assert 0.05 < r1 < r10 <= 1.0


def test_coco_shape_c3_depth1000(m, tmp_path):
    # COCO-5K t->i shape with the hybrid script's depth 1000 (scripts/search.sh:25): large-k path
    _case(m, tmp_path, 5000, 128, 300, 120, 30000, seed=2, tile_docs=0, ks=[10, 1000])


def test_coco_shape_c3_image_to_text_full(m, tmp_path):
    # BASELINE config 3, image->text direction at its real shape: 25 010 caption docs (4 tiles of 8192, the default
    # tile), ALL 5 000 image queries x 120 nnz, V = 30 000; top-10 (scripts/search_sparse.sh:22) and the hybrid
    # script's depth 1000 (scripts/search.sh:25), every query against the C oracle
    _case(m, tmp_path, 25010, 128, 5000, 120, 30000, seed=2, tile_docs=0, ks=[10, 1000])


def test_coco_shape_c3_text_to_image_full(m, tmp_path):
    # ... and the text->image direction with all 25 010 caption queries against 5 000 image docs (one tile)
    _case(m, tmp_path, 5000, 128, 25010, 120, 30000, seed=3, tile_docs=0, ks=[10])


def test_many_query_terms(m, tmp_path):
    # > 256 terms per query exercises the staged term rounds
    _case(m, tmp_path, 9000, 32, 50, 700, 4000, seed=5, tile_docs=4096, ks=[10, 37])


def test_heavy_ties_and_string_order(m, tmp_path):
    # every doc holds the same single term with the same weight -> all scores tie; order must be doc-id STRING order
    n, V = 10000, 8
    dp = np.arange(n + 1, dtype=np.uint64)
    dt = np.full(n, 3, dtype=np.uint32)
    dw = np.full(n, 7, dtype=np.uint32)
    dt[::2] = 4  # half the docs hold term 4 instead, so neither term has df == N
    ids = [str(i) for i in range(n)]
    path = m.build_index_from_csr(str(tmp_path / "t.idx"), dp, dt, dw, V, doc_ids=ids, tile_docs=4096)
    qp = np.array([0, 1, 3], dtype=np.int64)
    qt = np.array([3, 3, 4], dtype=np.int32)
    qw = np.array([2, 1, 1], dtype=np.int32)
    oix, _ = helpers.taat_oracle((dp, dt, dw), V, ids)
    with m.SparseIndex(path, device=0) as ix:
        for k in (1, 10, 300, 1000):
            got = ix.search_csr(qp, qt, qw, k)
            helpers.assert_same_results(got, oix.search(qp, qt, qw, k), k)
        ords, _, su, cnt = ix.search_csr(qp, qt, qw, 5)
        got_ids = ix.docids(ords[0, : cnt[0]])
    odd = sorted((str(i) for i in range(1, n, 2)), key=lambda s: s.encode())
    assert got_ids == odd[:5] and (su[0] == 14).all()


def test_edge_queries(m, tmp_path):
    docs, _ = helpers.synth(3000, 16, 1, 4, 500, seed=9)
    path = m.build_index_from_csr(str(tmp_path / "e.idx"), *docs, 500, tile_docs=4096)
    oix, _ = helpers.taat_oracle(docs, 500)
    # empty query, all-OOV query, zero/negative weights, duplicate terms (add), one ordinary query
    qp = np.array([0, 0, 2, 5, 8, 10], dtype=np.int64)
    qt = np.array([-1, -1, 7, 7, 9, 11, 11, 11, 3, 4], dtype=np.int32)
    qw = np.array([5, 9, 0, -3, 4, 2, 3, 1, 6, 2], dtype=np.int32)
    with m.SparseIndex(path, device=0) as ix:
        got = ix.search_csr(qp, qt, qw, 10)
        helpers.assert_same_results(got, oix.search(qp, qt, qw, 10), 10)
        assert got[3][0] == 0 and got[3][1] == 0
        # out-of-range term id and k are refused, not computed
        with pytest.raises(Exception):
            ix.search_csr(np.array([0, 1]), np.array([500]), np.array([1]), 10)
        with pytest.raises(Exception):
            ix.search_csr(qp, qt, qw, 2000)
        # nq = 0
        e = ix.search_csr(np.array([0]), np.array([], dtype=np.int32), np.array([], dtype=np.int32), 10)
        assert e[0].shape == (0, 10)


def test_big_batch_is_normalised_like_small_batches(m, tmp_path):
    # a batch of >= 8192 queries is normalised by several host threads (msr_device.hip, batch_create_impl); the result
    # must be the one of the single-threaded walk that small batches take, ragged/empty/OOV/duplicate queries included
    n_terms = 3000
    docs, (qp, qt, qw) = helpers.synth(6000, 48, 20011, 9, n_terms, seed=77)
    rng = np.random.default_rng(78)
    qt = qt.copy()
    qw = qw.copy()
    qt[rng.random(qt.size) < 0.05] = -1                      # OOV entries
    qw[rng.random(qw.size) < 0.05] = 0                       # dropped weights
    dup = rng.random(qt.size) < 0.05
    qt[1:][dup[1:]] = qt[:-1][dup[1:]]                       # repeated terms (weights add up)
    path = m.build_index_from_csr(str(tmp_path / "b.idx"), *docs, n_terms, tile_docs=4096)
    oix, _ = helpers.taat_oracle(docs, n_terms)
    with m.SparseIndex(path, device=0) as ix:
        big = ix.search_csr(qp, qt, qw, 10)
        step = 2500                                          # < 8192: the serial walk
        for a in range(0, 20011, step):
            b = min(a + step, 20011)
            sub = ix.search_csr(qp[a:b + 1] - qp[a], qt[qp[a]:qp[b]], qw[qp[a]:qp[b]], 10)
            for x, y in zip(big, sub):
                np.testing.assert_array_equal(x[a:b], y)
        sel = np.arange(0, 20011, 37)
        sp = np.concatenate([[0], np.cumsum(qp[sel + 1] - qp[sel])]).astype(np.int64)
        st = np.concatenate([qt[qp[i]:qp[i + 1]] for i in sel])
        sw = np.concatenate([qw[qp[i]:qp[i + 1]] for i in sel])
        want = oix.search(sp, st, sw, 10, threads=8)
        helpers.assert_same_results(tuple(x[sel] for x in big), want, 10)
        # two bad queries in different threads' ranges: the LOWEST one is reported, as a serial walk would
        bt = qt.copy()
        lo_q, hi_q = 9001, 19000
        assert qp[lo_q + 1] > qp[lo_q] and qp[hi_q + 1] > qp[hi_q]
        bt[qp[hi_q]] = n_terms + 5
        bt[qp[lo_q]] = n_terms + 7
        with pytest.raises(Exception, match=f"query {lo_q}: term id {n_terms + 7}"):
            ix.search_csr(qp, bt, qw, 10)
        bp = qp.copy()
        bp[15000] = bp[15001] + 1                            # not monotone
        with pytest.raises(Exception, match="not monotone"):
            ix.search_csr(bp, qt, qw, 10)


def test_df_eq_n_switch(m, tmp_path):
    # term 0 is in every doc: dropped by default (contract T3), kept when the switch is off
    n, V = 500, 20
    rng = np.random.default_rng(5)
    rows = [[(0, int(rng.integers(1, 50)))] + [(int(t), int(rng.integers(1, 50))) for t in rng.choice(np.arange(1, V), 3, replace=False)]
            for _ in range(n)]
    dp = np.arange(0, 4 * n + 1, 4, dtype=np.uint64)
    dt = np.array([t for r in rows for t, _ in r], dtype=np.uint32)
    dw = np.array([w for r in rows for _, w in r], dtype=np.uint32)
    path = m.build_index_from_csr(str(tmp_path / "d.idx"), dp, dt, dw, V, tile_docs=4096)
    oix, _ = helpers.taat_oracle((dp, dt, dw), V)
    qp = np.array([0, 2, 3], dtype=np.int64)
    qt = np.array([0, 5, 0], dtype=np.int32)
    qw = np.array([3, 2, 1], dtype=np.int32)
    with m.SparseIndex(path, device=0) as ix:
        for drop in (True, False):
            got = ix.search_csr(qp, qt, qw, 10, drop_df_eq_n=drop)
            helpers.assert_same_results(got, oix.search(qp, qt, qw, 10, drop_df_eq_n=drop), 10)
        assert ix.search_csr(qp, qt, qw, 10, drop_df_eq_n=True)[3][1] == 0


def test_overflow_is_refused(m, tmp_path):
    dp = np.array([0, 1, 2], dtype=np.uint64)
    dt = np.array([0, 1], dtype=np.uint32)
    dw = np.array([65535, 65535], dtype=np.uint32)
    path = m.build_index_from_csr(str(tmp_path / "o.idx"), dp, dt, dw, 2, tile_docs=4096)
    with m.SparseIndex(path, device=0) as ix:
        with pytest.raises(Exception, match="OVERFLOW|RANGE"):
            ix.search_csr(np.array([0, 1]), np.array([0]), np.array([70000]), 1)
        ords, f32, u32, n = ix.search_csr(np.array([0, 1]), np.array([0]), np.array([65535]), 1)
        assert n[0] == 1 and u32[0, 0] == 65535 * 65535 and f32[0, 0] == np.float32(65535 * 65535)


def test_resident_batch_and_shards(m, tmp_path):
    # doc-range shards searched one by one on the same GPU, merged by msr_merge_lists == unsharded result
    docs, (qp, qt, qw) = helpers.synth(30000, 32, 300, 30, 3000, seed=31)
    path = m.build_index_from_csr(str(tmp_path / "s.idx"), *docs, 3000, tile_docs=4096)
    oix, _ = helpers.taat_oracle(docs, 3000)
    want = oix.search(qp, qt, qw, 10, threads=8)
    with m.SparseIndex(path, device=0) as ix:
        b = ix.batch(qp, qt, qw, 16)
        b.search(10)
        helpers.assert_same_results(b.fetch(), want, 10)
        ms = b.kernel_ms()
        by, po = b.algo_bytes(10)
        assert ms[0] > 0 and by > po * 6
        b.close()
        lists = []
        for s in range(3):
            with m.SparseIndex(path, device=0, shard=s, n_shards=3) as sh:
                assert sh.shard_ntiles in (2, 3)
                lists.append(sh.search_csr(qp, qt, qw, 10))
        o, sf, su, n = ix.merge_lists(np.stack([l[0] for l in lists]), np.stack([l[2] for l in lists]),
                                      np.stack([l[3] for l in lists]), 10)
        helpers.assert_same_results((o, sf, su, n), want, 10)


def test_two_threads_two_handles(m, tmp_path):
    # handles are not thread-safe, but two threads with a handle EACH may search at the same time (ctypes releases the
    # GIL during the calls: the two streams, staging buffers and error strings must not meet)
    import threading

    docs, (qp, qt, qw) = helpers.synth(20000, 48, 400, 30, 3000, seed=61)
    path = m.build_index_from_csr(str(tmp_path / "t.idx"), *docs, 3000, tile_docs=4096)
    oix, _ = helpers.taat_oracle(docs, 3000)
    want = {k: oix.search(qp, qt, qw, k, threads=8) for k in (10, 100)}
    errors = []

    def work(k):
        try:
            with m.SparseIndex(path, device=0) as ix:
                for _ in range(20):
                    helpers.assert_same_results(ix.search_csr(qp, qt, qw, k), want[k], k)
                with pytest.raises(Exception, match="outside the dictionary"):   # an error in one thread stays there
                    ix.search_csr(np.array([0, 1]), np.array([3000]), np.array([1]), k)
        except BaseException as e:  # noqa: BLE001 (reported by the main thread)
            errors.append(e)

    ts = [threading.Thread(target=work, args=(k,)) for k in (10, 100, 10, 100)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors


def test_rccl_single_rank(m, tmp_path):
    # the RCCL exchange path with a 1-rank communicator (all a 1-GPU box can run)
    docs, (qp, qt, qw) = helpers.synth(12000, 32, 100, 30, 3000, seed=41)
    path = m.build_index_from_csr(str(tmp_path / "r.idx"), *docs, 3000, tile_docs=4096)
    oix, _ = helpers.taat_oracle(docs, 3000)
    with m.SparseIndex(path, device=0) as ix:
        ix.comm_init(1, 0, m.comm_unique_id())
        b = ix.batch(qp, qt, qw, 10)
        b.search(10, sharded=True)
        helpers.assert_same_results(b.fetch(), oix.search(qp, qt, qw, 10), 10)
        b.close()
        ix.comm_destroy()


# ------------------------------------------------------------------------------------------------ golden fixture
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_golden_fixture_through_the_dropin_class(m, tmp_path):
    """corpus jsonl -> index -> LuceneImpactSearcher.batch_search -> sparse_search/get_run_dict, as src/search.py
    drives it; expected hits are the committed fixture (oracle-generated: parity unpinned, see the fixture's README)."""
    import json
    import shutil
    from types import SimpleNamespace

    from mllm_sparse_retrieval_amd.compat import JWhiteSpaceAnalyzer, LuceneImpactSearcher, get_run_dict, sparse_search

    work = tmp_path / "enc"
    shutil.copytree(os.path.join(GOLD, "sparse_small"), work)
    m.build_index_from_jsonl(str(work), threads=4)                       # -> work/index/msr.idx
    exp = json.load(open(os.path.join(GOLD, "sparse_small_expected.json")))
    queries = [line.rstrip("\n").split("\t") for line in open(work / "query.tsv", encoding="utf-8")]
    qids, texts = [q for q, _ in queries], [t for _, t in queries]
    r = LuceneImpactSearcher(os.path.join(str(work), "index"), None)
    r.set_analyzer(JWhiteSpaceAnalyzer())
    for k in (3, 10, 100):
        scores, rankings = sparse_search(r, texts, qids, SimpleNamespace(depth=k, threads=16))
        want = exp["cases"][f"drop=1,k={k}"]
        for qid, sc, rk in zip(qids, scores, rankings):
            assert rk == [d for d, _ in want[qid]], (k, qid)
            assert sc == [float(s) for _, s in want[qid]]
    run = get_run_dict(qids, scores, rankings, remove_query=True)
    assert "9" not in run["9"]["docs"] and run["1003"]["docs"] == {}
    # min_idf < 0 switches the df == N filter off (contract T3 switch)
    r2 = LuceneImpactSearcher(os.path.join(str(work), "index"), None, min_idf=-1)
    hits = r2.batch_search(["the the"], ["x"], 3)["x"]
    assert [(h.docid, h.score) for h in hits] == [(d, float(s)) for d, s in exp["cases"]["drop=0,k=3"]["1004"]]
    r.close()
    r2.close()


def test_cli_search_end_to_end(m, tmp_path, capsys):
    from mllm_sparse_retrieval_amd import cli
    from mllm_sparse_retrieval_amd.fusion import read_trec_run

    enc = str(tmp_path / "enc")
    cli.main(["encode", "--synthetic", "flickr", "--n_images", "300", "--sparse_output_dir", enc, "--threads", "4"])
    cli.main(["index", "--input", enc, "--threads", "4", "--impact", "--pretokenized"])
    cli.main(["search", "--sparse_index", enc, "--depth", "10", "--threads", "16", "--batch_size", "256",
              "--query_type", "text", "--dataset_name", "flickr", "--qrels", os.path.join(enc, "qrels.csv"),
              "--save_dir", str(tmp_path / "runs"), "--remove_query"])
    out = capsys.readouterr().out
    line = [l for l in out.splitlines() if l.startswith("Sparse reps recall")][0]
    r1 = float(line.split("r@1 ")[1].split(",")[0])
    assert 0.2 < r1 <= 1.0                                               # planted signal is found
    run = read_trec_run(str(tmp_path / "runs" / "sparse.trec"))
    assert len(run) == 1500 and all(len(v["docs"]) <= 10 for v in run.values())
    # hybrid: dense reps next to the sparse files, --passage_reps switches dense + fusion on (scripts/search.sh)
    dense = str(tmp_path / "dense")
    cli.main(["encode", "--synthetic", "flickr", "--n_images", "300", "--sparse_output_dir", enc, "--threads", "4",
              "--dense_output_dir", dense, "--dense_dim", "64"])
    cli.main(["search", "--sparse_index", enc, "--passage_reps", dense, "--depth", "100", "--batch_size", "500",
              "--alpha", "0.5", "--query_type", "text", "--dataset_name", "flickr",
              "--qrels", os.path.join(enc, "qrels.csv"), "--save_dir", str(tmp_path / "runs2")])
    out = capsys.readouterr().out
    rec = {name: float([l for l in out.splitlines() if l.startswith(name)][0].split("r@10 ")[1].split(",")[0])
           for name in ("Dense reps recall", "Sparse reps recall", "Fusion/Hybrid reps recall")}
    assert rec["Fusion/Hybrid reps recall"] >= max(rec["Dense reps recall"], rec["Sparse reps recall"]) - 0.02
    assert os.path.exists(tmp_path / "runs2" / "fusion.trec")
    # that was ONE msr_hybrid_search call over the query file; --host_fusion is the reference's own structure (lists per
    # batch + fuse() on the host, src/search.py:455-461): the same report, the same runs
    recall_lines = [l for l in out.splitlines() if "recall" in l]
    cli.main(["search", "--sparse_index", enc, "--passage_reps", dense, "--depth", "100", "--batch_size", "500",
              "--alpha", "0.5", "--query_type", "text", "--dataset_name", "flickr", "--host_fusion",
              "--qrels", os.path.join(enc, "qrels.csv"), "--save_dir", str(tmp_path / "runs3")])
    out3 = capsys.readouterr().out
    assert [l for l in out3.splitlines() if "recall" in l] == recall_lines
    for name in ("sparse.trec", "dense.trec"):
        a, b = read_trec_run(str(tmp_path / "runs2" / name)), read_trec_run(str(tmp_path / "runs3" / name))
        assert a.keys() == b.keys()
        assert all(list(a[q]["docs"]) == list(b[q]["docs"]) for q in a), name
    fa, fb = read_trec_run(str(tmp_path / "runs2" / "fusion.trec")), read_trec_run(str(tmp_path / "runs3" / "fusion.trec"))
    for q in fb:   # the GPU run keeps the best --fusion_k of the union; scores within 1e-5, order equal up to near-ties
        da, db = fa[q]["docs"], fb[q]["docs"]
        assert set(da) <= set(db) and len(da) == min(len(db), 1000)
        assert max(abs(da[d] - db[d]) for d in da) <= 1e-5
        ra, rb = list(da)[:10], list(db)[:10]
        assert all(x == y or abs(db[x] - db[y]) <= 2e-6 for x, y in zip(ra, rb))


@pytest.mark.parametrize("query_type", ["image", "text"])
def test_cli_on_the_reference_coco_ids(m, tmp_path, capsys, query_type):
    """index -> search --qrels -> eval on a synthetic corpus KEYED TO THE IDS OF THE REFERENCE'S COCO-5K TEST SPLIT
    (tests/golden/coco_test_ids.csv = the id columns of data/coco/coco_test.csv): docs are named by real caption ids (2-6
    digits: ordinals follow the id STRING order, contract T1) or real image ids (sparse, 0 .. 40 503), image queries have
    5 or 6 target captions (any-of-N get_target, src/dataset.py:164-168, src/metrices.py:76-84), and 149 ids exist on both
    sides, so --remove_query (scripts/search_sparse.sh:26) removes real docs. The TREC run must equal the oracle's hits
    under those ids, and the printed recall an independent count."""
    import json

    from mllm_sparse_retrieval_amd import cli
    from mllm_sparse_retrieval_amd.fusion import read_trec_run
    from mllm_sparse_retrieval_amd.qrels import CrossModalQrels

    ds = CrossModalQrels(os.path.join(os.path.dirname(__file__), "golden", "coco_test_ids.csv"), "coco")
    assert len(ds.img_id_list) == 5000 and len(ds.text_id_list) == 25010
    assert sorted(len(v) for v in ds.img2text.values())[-10:] == [6] * 10 and len(set(ds.img_id_list) & set(ds.text_id_list)) == 149
    n_terms, k = 3000, 10
    if query_type == "image":   # image -> text: docs = captions, queries = images
        doc_ids, query_ids = ds.text_id_list, ds.img_id_list[:1500]
        owner = {t: i for i, ts in ds.img2text.items() for t in ts}
        pair_of_doc = [owner[d] for d in doc_ids]
    else:                       # text -> image: docs = images, queries = captions
        doc_ids, query_ids = ds.img_id_list, ds.text_id_list[:3000]
        pair_of_doc = doc_ids
    # synthetic vectors with planted signal: a caption and its image share 8 terms; tokens are 't<id>'
    img_index = {i: j for j, i in enumerate(ds.img_id_list)}
    base = m.synth_vectors(5000, 8, n_terms, seed=77, threads=8)                # the shared terms of every image
    bt, bw = base[1].reshape(5000, 8), base[2].reshape(5000, 8)
    fill_d = m.synth_vectors(len(doc_ids), 24, n_terms, seed=78, threads=8)
    fill_q = m.synth_vectors(len(query_ids), 8, n_terms, seed=79, threads=8)
    enc = tmp_path / "enc"
    enc.mkdir()
    doc_rows = []
    with open(enc / "corpus_0.jsonl", "w") as f:
        for j, d in enumerate(doc_ids):
            img = img_index[pair_of_doc[j]]
            vec = {f"t{int(t)}": int(w) for t, w in zip(fill_d[1][24 * j:24 * j + 24], fill_d[2][24 * j:24 * j + 24])}
            vec.update({f"t{int(t)}": int(w) for t, w in zip(bt[img], bw[img])})
            if query_type == "image" and d in img_index:
                # this caption's id is ALSO an image id: let it match that image's query too, so that the query finds
                # "itself" among its hits and --remove_query has a real doc to remove
                vec.update({f"t{int(t)}": int(w) + 50 for t, w in zip(bt[img_index[d]], bw[img_index[d]])})
            doc_rows.append(vec)
            f.write(json.dumps(dict(id=d, content="", vector=vec)) + "\n")
    q_rows = []
    with open(enc / "query.tsv", "w") as f:
        for j, qid in enumerate(query_ids):
            img = img_index[qid if query_type == "image" else ds.text2img[qid]]
            vec = {f"t{int(t)}": int(w) for t, w in zip(fill_q[1][8 * j:8 * j + 8], fill_q[2][8 * j:8 * j + 8])}
            vec.update({f"t{int(t)}": int(w) for t, w in zip(bt[img], bw[img])})
            q_rows.append(vec)
            f.write(qid + "\t" + " ".join(" ".join([tok] * w) for tok, w in vec.items()) + "\n")
    qrels = os.path.join(os.path.dirname(__file__), "golden", "coco_test_ids.csv")
    cli.main(["index", "--input", str(enc), "--threads", "8"])
    cli.main(["search", "--sparse_index", str(enc), "--depth", str(k), "--batch_size", "512", "--query_type", query_type,
              "--dataset_name", "coco", "--qrels", qrels, "--save_dir", str(tmp_path / "runs"), "--remove_query"])
    out = capsys.readouterr().out
    line = [l for l in out.splitlines() if l.startswith("Sparse reps recall")][0]
    printed = [float(x.split()[1].rstrip(",")) for x in line.split("r@")[1:]][:3]      # r@1, r@5, r@10
    run = read_trec_run(str(tmp_path / "runs" / "sparse.trec"))
    # the oracle under the same ids (ordinals = ranks of the id STRINGS)
    vocab = sorted({t for v in doc_rows for t in v})
    tid = {t: i for i, t in enumerate(vocab)}
    dp = np.concatenate([[0], np.cumsum([len(v) for v in doc_rows])]).astype(np.uint64)
    dt = np.array([tid[t] for v in doc_rows for t in v], dtype=np.uint32)
    dw = np.array([w for v in doc_rows for w in v.values()], dtype=np.uint32)
    oix, order = helpers.taat_oracle((dp, dt, dw), len(vocab), doc_ids)
    sorted_ids = [doc_ids[r] for r in order]
    assert sorted_ids == sorted(doc_ids, key=lambda x: x.encode()) and sorted_ids != sorted(doc_ids, key=int)
    qp = np.concatenate([[0], np.cumsum([len(v) for v in q_rows])]).astype(np.int64)
    qt = np.array([tid.get(t, -1) for v in q_rows for t in v], dtype=np.int32)
    qw = np.array([w for v in q_rows for w in v.values()], dtype=np.int32)
    wo, ws, wn = oix.search(qp, qt, qw, k, threads=8)
    hits = {1: 0, 5: 0, 10: 0}
    removed = 0
    for j, qid in enumerate(query_ids):
        want = [(sorted_ids[int(o)], float(s)) for o, s in zip(wo[j, :wn[j]], ws[j, :wn[j]])]
        removed += any(d == qid for d, _ in want)
        want = [(d, s) for d, s in want if d != qid]                                   # remove_query, src/search.py:72-74
        got = list(run[qid]["docs"].items())
        assert got == want, (qid, got[:3], want[:3])
        target = ds.get_target(qid, query_type)
        tset = set(target) if isinstance(target, list) else {target}
        ranked = [d for d, _ in sorted(want, key=lambda kv: -kv[1])]                    # (stable: ties keep hit order)
        for kk in hits:
            hits[kk] += bool(tset & set(ranked[:kk]))
    assert printed == pytest.approx([hits[kk] / len(query_ids) for kk in (1, 5, 10)], abs=1e-12)
    assert printed[2] > 0.5                                                             # the planted signal is found
    if query_type == "image":
        assert removed > 0                                                             # a real id lives on both sides
    # the stand-alone recall reporter over the TREC run gives the same numbers
    cli.main(["eval", "--runs_dir", str(tmp_path / "runs"), "--qrels", qrels, "--dataset_name", "coco", "--query_type",
              query_type, "--queries", str(enc / "query.tsv")])
    line2 = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Sparse reps recall")][0]
    assert line2 == line


def _free_port():
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_cli_search_two_ranks_dp_over_queries(m, tmp_path):
    """`search` under a launcher = the reference's DP over queries (src/search.py:115-129,180-182; launcher line
    scripts/search_sparse.sh:14): two ranks (sharing this box's one GPU), each searches its DistributedSampler shard, only
    recall fractions are gathered. The merged TREC run equals the single-process run, the summed recall equals the
    single-process recall (true denominator), and --compat-denominator reproduces the padded denominator."""
    import subprocess
    import sys

    from mllm_sparse_retrieval_amd import cli

    enc = str(tmp_path / "enc")
    cli.main(["encode", "--synthetic", "flickr", "--n_images", "201", "--sparse_output_dir", enc, "--threads", "4"])
    cli.main(["index", "--input", enc, "--threads", "4"])
    common = ["--sparse_index", enc, "--depth", "10", "--batch_size", "128", "--query_type", "text", "--dataset_name",
              "flickr", "--qrels", os.path.join(enc, "qrels.csv")]

    def run(world, extra, save):
        env = dict(os.environ, MSR_SHARE_GPU="1", PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        for k2 in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
            env.pop(k2, None)
        cmd = [sys.executable] + (["-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr",
                                   "127.0.0.1", "--master-port", str(_free_port()), "-m", "mllm_sparse_retrieval_amd"]
                                  if world > 1 else ["-m", "mllm_sparse_retrieval_amd"])
        p = subprocess.run(cmd + ["search"] + common + ["--save_dir", save] + extra, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, env=env, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-3000:]
        # (without the timing line and gloo's connection banner — two ranks write the banner to the same pipe, so a
        # line of it can arrive in pieces)
        return [x for x in p.stdout.decode().splitlines()
                if not x.startswith("search:") and "[Gloo]" not in x and "peer ranks" not in x and x.strip()]

    one = run(1, [], str(tmp_path / "r1"))
    two = run(2, [], str(tmp_path / "r2"))
    compat = run(2, ["--compat-denominator"], str(tmp_path / "r3"))
    n = 201 * 5                                                                   # 1005 captions: odd -> one padded repeat
    assert one[0] == str(n) and two[0] == str(n) and compat[0] == str(n + 1)

    def summary(lines):
        line = [x for x in lines if x.startswith("Sparse reps recall")][0]
        return [float(x.split()[1].rstrip(",")) for x in line.split("r@")[1:]]

    assert np.allclose(summary(one), summary(two), atol=1e-12)
    per_rank = [x for x in two if x.startswith("Sparse recall @ 1:")][0]
    assert per_rank.count(",") == 1                                               # two ranks' fractions
    assert abs(summary(compat)[0] * (n + 1) - summary(one)[0] * n) <= 1 + 1e-9   # the repeat counts at most once more
    a = sorted(open(tmp_path / "r1" / "sparse.trec").read().splitlines())
    b = sorted(open(tmp_path / "r2" / "sparse.trec").read().splitlines())
    assert a == b and len(a) > 9000
    assert not os.path.exists(tmp_path / "r2" / "sparse.trec.rank0")


# ------------------------------------------------------------------------------------------------ full-size properties
@pytest.mark.parametrize("tile_docs,n_tiles", [(32768, 31), (0, 123)])
def test_full_size_properties_c4(m, tmp_path, tile_docs, n_tiles):
    """BASELINE config 4 size (1 M docs, 128 M postings): size-independent properties instead of a full oracle run,
    plus an oracle check on a query sample. tile_docs = 0 is the production instance bench.py runs (8192-doc tiles,
    123 tiles, staged search with 7 first-stage tiles)."""
    n_docs, n_terms, nq = 1_000_000, 30000, 2000
    docs = m.synth_vectors(n_docs, 128, n_terms, seed=3, threads=16)
    qp, qt, qw = m.synth_vectors(nq, 120, n_terms, seed=4, threads=16)
    qp, qt, qw = qp.astype(np.int64), qt.astype(np.int32), qw.astype(np.int32)
    path = m.build_index_from_csr(str(tmp_path / "c4.idx"), *docs, n_terms, tile_docs=tile_docs)
    with m.SparseIndex(path, device=0) as ix:
        assert ix.n_tiles == n_tiles and ix.n_postings == 128_000_000
        o, f, u, n = ix.search_csr(qp, qt, qw, 10)
        assert (n == 10).all()
        assert (np.diff(u.astype(np.int64), axis=1) <= 0).all()                       # sorted by score
        tie = np.diff(u.astype(np.int64), axis=1) == 0
        assert (np.diff(o.astype(np.int64), axis=1)[tie] > 0).all()                   # ties by ordinal
        assert (f == u.astype(np.float32)).all() and (o < n_docs).all()
        # linearity: doubling every query weight doubles every score and keeps the ranking
        o2, _, u2, _ = ix.search_csr(qp, qt, qw * 2, 10)
        assert (o2 == o).all() and (u2 == 2 * u).all()
        # idempotence / prefix property: top-3 is the prefix of top-10; a second run is identical
        o3, _, u3, _ = ix.search_csr(qp, qt, qw, 3)
        assert (o3 == o[:, :3]).all() and (u3 == u[:, :3]).all()
        # shard decomposition: merging 4 doc-range shards' exact top-k equals the unsharded answer
        lists = []
        for s in range(4):
            with m.SparseIndex(path, device=0, shard=s, n_shards=4) as sh:
                lists.append(sh.search_csr(qp, qt, qw, 10))
        mo, _, mu, mn = ix.merge_lists(np.stack([l[0] for l in lists]), np.stack([l[2] for l in lists]),
                                       np.stack([l[3] for l in lists]), 10)
        assert (mo == o).all() and (mu == u).all() and (mn == n).all()
    if tile_docs == 0:
        # the north star's TERM-range partition at config-4 size (BASELINE.json configs[3]): G = 8 handles,
        # each resident with its own term range of all 123 tiles only, play the exact protocol on this one GPU — every
        # shard dumps its partial accumulator tiles (two passes of 1 024 queries through the 4 GiB buffer), the sums of
        # each doc range are selected (16 tiles per range), the range lists merged: identical to the doc-range result
        from mllm_sparse_retrieval_amd.index import search_termshard_emulated_handles

        shards = [m.SparseIndex(path, device=0, term_shard=(g, 8)) for g in range(8)]
        try:
            assert [sh.term_lo for sh in shards[1:]] == [sh.term_hi for sh in shards[:-1]]
            assert shards[0].term_lo == 0 and shards[-1].term_hi == n_terms
            whole = sum(sh.resident_bytes for sh in shards)
            with m.SparseIndex(path, device=0) as full:
                assert whole < 1.25 * full.resident_bytes          # nothing replicated but shared dense-head pairs
            to, tf, tu, tn = search_termshard_emulated_handles(shards, qp, qt, qw, 10)
            assert (to == o).all() and (tu == u).all() and (tf == f).all() and (tn == n).all()
        finally:
            for sh in shards:
                sh.close()
    # oracle on a sample of the same queries
    oix, _ = helpers.taat_oracle(docs, n_terms)
    s = 200
    want = oix.search(qp[: s + 1], qt[: qp[s]], qw[: qp[s]], 10, threads=16)
    helpers.assert_same_results((o[:s], f[:s], u[:s], n[:s]), want, 10)


def test_staged_search_thresholds(m, tmp_path):
    """The staged search (first tiles -> per-query threshold -> remaining tiles report only keys at or above it):
    hits that exist only in the last tile (no threshold from the first stage), a first stage that is beaten by every
    later tile, exact score ties straddling the stage boundary (the lower ordinal of the first tile must win), and
    thresholds that admit more survivors than the candidate buffer (fallback to the full per-tile selection)."""
    tile, n_tiles = 4096, 20
    n, V = tile * n_tiles, 12
    rows_t, rows_w, ptr = [], [], [0]
    rng = np.random.default_rng(5)
    for d in range(n):
        t_id = d // tile
        terms, ws = [], []
        if t_id == n_tiles - 1:            # term 0: only in the last tile
            terms.append(0); ws.append(1 + d % 7)
        terms.append(1); ws.append(1 + t_id)           # term 1: weight grows with the tile -> later tiles always win
        terms.append(2); ws.append(5)                   # term 2: the same weight everywhere -> all scores tie
        if d % 3 == 0:
            terms.append(3); ws.append(int(rng.integers(1, 400)))  # term 3: random
        terms.append(4 + d % 4); ws.append(2)           # terms 4-7: a quarter of the docs each, equal weights
        rows_t += terms; rows_w += ws; ptr.append(len(rows_t))
    docs = (np.array(ptr, dtype=np.uint64), np.array(rows_t, dtype=np.uint32), np.array(rows_w, dtype=np.uint32))
    m.set_build_option("dense_max_terms", 0)
    try:
        path = m.build_index_from_csr(str(tmp_path / "s.idx"), *docs, V, tile_docs=tile)
    finally:
        m.set_build_option("dense_max_terms", 16)
    queries = [[(0, 3)], [(1, 2)], [(2, 9)], [(3, 1), (2, 1)], [(4, 1)], [(1, 1), (3, 2), (5, 7)], [(0, 1), (2, 1)]]
    queries = queries * 40  # 280 queries x 20 tiles: above the library's minimum of (tile, query) pairs for staging
    qp = np.cumsum([0] + [len(q) for q in queries]).astype(np.int64)
    qt = np.array([t for q in queries for t, _ in q], dtype=np.int32)
    qw = np.array([w for q in queries for _, w in q], dtype=np.int32)
    oix, _ = helpers.taat_oracle(docs, V)
    with m.SparseIndex(path, device=0) as ix:
        assert ix.n_tiles == n_tiles
        for k in (1, 10, 64, 100, 600, 1024):
            for drop in (False, True):
                helpers.assert_same_results(ix.search_csr(qp, qt, qw, k, drop_df_eq_n=drop),
                                            oix.search(qp, qt, qw, k, drop_df_eq_n=drop), k)


def test_merge_of_many_tile_lists(m, tmp_path):
    # 37 tiles x k=100 = 3 700 partial keys per query: more than the merge kernel's LDS buffer, so the list-head
    # threshold path (and, with k = 1000 > #lists, the full bisection) is exercised
    _case(m, tmp_path, 150000, 16, 120, 30, 2000, seed=77, tile_docs=4096, ks=[10, 100, 1000])


@pytest.mark.parametrize("tile_docs", [4096, 8192])
def test_term_range_shards_emulated(m, tmp_path, tile_docs):
    # the term-sharded protocol (dump accumulators -> sum -> select per doc range -> merge) for G logical shards on
    # one GPU must reproduce the unsharded answer exactly; 30 000 docs = 8 / 4 tiles, not divisible by every G
    docs, (qp, qt, qw) = helpers.synth(30000, 48, 150, 40, 3000, seed=91)
    path = m.build_index_from_csr(str(tmp_path / "t.idx"), *docs, 3000, tile_docs=tile_docs)
    oix, _ = helpers.taat_oracle(docs, 3000)
    with m.SparseIndex(path, device=0) as ix:
        for k in (10, 100):
            want = oix.search(qp, qt, qw, k, threads=8)
            for g in (1, 2, 3, 8):
                helpers.assert_same_results(ix.search_termshard_emulated(qp, qt, qw, k, g), want, k)
        # a doc-range shard handle cannot run the term protocol
        with m.SparseIndex(path, device=0, shard=0, n_shards=2) as sh:
            with pytest.raises(Exception, match="every doc tile"):
                sh.search_termshard_emulated(qp, qt, qw, 10, 2)


@pytest.mark.parametrize("tile_docs,dense_max", [(4096, 16), (8192, 16), (4096, 0), (4096, 5)])
def test_term_range_shard_handles_hold_only_their_terms(m, tmp_path, tile_docs, dense_max):
    """msr_index_open_termshard: G handles, each resident with ONLY its term range (segment-table columns, postings
    slices, the dense-head pairs holding an owned term); the protocol played over them == the unsharded oracle
    result; the per-shard resident postings add up to the whole index; misuse is refused."""
    docs, (qp, qt, qw) = helpers.synth(30000, 48, 150, 40, 3000, seed=91)
    m.set_build_option("dense_max_terms", dense_max)
    try:
        path = m.build_index_from_csr(str(tmp_path / "t.idx"), *docs, 3000, tile_docs=tile_docs)
    finally:
        m.set_build_option("dense_max_terms", 16)
    oix, _ = helpers.taat_oracle(docs, 3000)
    with m.SparseIndex(path, device=0) as full:
        seg_table = full.n_tiles * (full.n_terms + 1) * 4
        dense_bytes = full.n_tiles * (full.n_dense // 2) * full.tile_docs * 4
        post_bytes = full.resident_bytes - seg_table - dense_bytes
        for G in (1, 2, 3, 8):
            shards = [m.SparseIndex(path, device=0, term_shard=(g, G)) for g in range(G)]
            try:
                assert shards[0].term_lo == 0 and shards[-1].term_hi == 3000
                assert all(a.term_hi == b.term_lo for a, b in zip(shards, shards[1:]))
                # postings are partitioned: the shards' slices add up to the index's postings, nothing is replicated
                part = [sh.resident_bytes - sh.n_tiles * (sh.term_hi - sh.term_lo + 1) * 4 for sh in shards]
                assert sum(part) >= post_bytes and all(x <= post_bytes + dense_bytes for x in part)
                if G > 1:
                    assert max(sh.resident_bytes for sh in shards) < full.resident_bytes
                for k in (10, 100):
                    want = oix.search(qp, qt, qw, k, threads=8)
                    helpers.assert_same_results(m.search_termshard_emulated_handles(shards, qp, qt, qw, k), want, k)
                if G > 1:
                    with pytest.raises(Exception, match="term shard"):   # partial sums are not a search result
                        shards[1].search_csr(qp, qt, qw, 10)
                    with pytest.raises(Exception, match="term shard"):   # handles in the wrong order
                        m.search_termshard_emulated_handles(shards[::-1], qp, qt, qw, 10)
            finally:
                for sh in shards:
                    sh.close()


def test_term_shard_handle_rccl_single_rank(m, tmp_path):
    docs, (qp, qt, qw) = helpers.synth(20000, 32, 80, 30, 3000, seed=93)
    path = m.build_index_from_csr(str(tmp_path / "t1.idx"), *docs, 3000, tile_docs=4096)
    oix, _ = helpers.taat_oracle(docs, 3000)
    with m.SparseIndex(path, device=0, term_shard=(0, 1)) as ix:
        ix.comm_init(1, 0, m.comm_unique_id())
        assert ix.comm_info()[:2] == (1, 0)
        b = ix.batch(qp, qt, qw, 10)
        b.search(10, sharded="terms")
        helpers.assert_same_results(b.fetch(), oix.search(qp, qt, qw, 10), 10)
        with pytest.raises(Exception, match="term shard"):
            b.search(10, sharded=True)
        b.close()
        ix.comm_destroy()


def test_batch_outlives_its_index(m, tmp_path):
    """Closing the index first (e.g. an assert between ix.batch() and b.close()) must not turn into a crash: the
    batch is detached, refuses further use, and destroying it later only frees the host object."""
    docs, (qp, qt, qw) = helpers.synth(5000, 16, 20, 10, 500, seed=7)
    path = m.build_index_from_csr(str(tmp_path / "l.idx"), *docs, 500, tile_docs=4096)
    ix = m.SparseIndex(path, device=0)
    b1, b2 = ix.batch(qp, qt, qw, 10), ix.batch(qp, qt, qw, 10)
    b1.search(10)
    b2.search(10)
    want = b1.fetch()
    b2.close()                      # ordinary order for one of them
    ix.close()                      # ... and the index goes before b1
    with pytest.raises(Exception, match="closed"):
        b1.search(10)
    with pytest.raises(Exception, match="closed"):
        b1.fetch()
    b1.close()
    b1.close()                      # idempotent
    with m.SparseIndex(path, device=0) as ix2:   # the device is fine afterwards
        got = ix2.search_csr(qp, qt, qw, 10)
        assert all((a == b).all() for a, b in zip(got, want))


def test_term_range_shards_rccl_single_rank(m, tmp_path):
    docs, (qp, qt, qw) = helpers.synth(20000, 32, 80, 30, 3000, seed=93)
    path = m.build_index_from_csr(str(tmp_path / "t1.idx"), *docs, 3000, tile_docs=4096)
    oix, _ = helpers.taat_oracle(docs, 3000)
    with m.SparseIndex(path, device=0) as ix:
        ix.comm_init(1, 0, m.comm_unique_id())
        b = ix.batch(qp, qt, qw, 10, term_shard=(0, 1))
        b.search(10, sharded="terms")
        helpers.assert_same_results(b.fetch(), oix.search(qp, qt, qw, 10), 10)
        b.close()
        # a batch made for another partition is refused
        b2 = ix.batch(qp, qt, qw, 10, term_shard=(1, 2))
        with pytest.raises(Exception, match="term shard"):
            b2.search(10, sharded="terms")
        b2.close()
        ix.comm_destroy()


# ------------------------------------------------------------------------------------------------ dense / hybrid
def _unit_rows(rng, n, h):
    x = rng.standard_normal((n, h)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


_dense_oracle = helpers.dense_oracle


# (the last three cases fill >= 256 blocks of 256 x 256: the four-wave 16x16x32 GEMM kernel with 1, 2 and 3 steps of 64
# in K, a doc count that is not a multiple of the 4-doc store width, ragged last blocks in both directions; the others
# take the 128 x 128 kernel)
@pytest.mark.parametrize("n,h,nq,k", [(5000, 256, 300, 1000), (700, 64, 130, 10), (20000, 128, 64, 100), (3, 16, 5, 10),
                                      (4200, 192, 4100, 10), (9000, 64, 2100, 100), (4203, 128, 4100, 10)])
def test_dense_search_against_numpy(m, n, h, nq, k):
    from mllm_sparse_retrieval_amd.dense import FaissFlatSearcher

    rng = np.random.default_rng(n + h)
    p, q = _unit_rows(rng, n, h), _unit_rows(rng, nq, h)
    r = FaissFlatSearcher(p)
    r.add(p)
    # (batch_search issues one GPU call per batch: the big cases go in one call, the others in ragged batches of 97)
    scores, idx = r.batch_search(q, k, batch_size=nq if nq >= 2000 else 97, quiet=True)
    ws, wi = _dense_oracle(q, p, min(k, n))
    kk = min(k, n)
    assert np.abs(scores[:, :kk] - ws).max() <= 1e-5
    assert (idx[:, kk:] == -1).all() and np.isneginf(scores[:, kk:]).all()
    # row indices agree except where two scores are closer than the f32 accumulation noise
    diff = idx[:, :kk] != wi
    if diff.any():
        gap = np.abs(ws - np.take_along_axis(q.astype(np.float16).astype(np.float32)
                                             @ p.astype(np.float16).astype(np.float32).T, idx[:, :kk], axis=1))
        assert gap[diff].max() <= 2e-6 and diff.mean() < 0.01
    assert (np.diff(scores[:, :kk], axis=1) <= 0).all()


def test_dense_search_steady_state_allocates_nothing(m):
    """msr_dense_search keeps its device scratch and events on the handle: after the first call of a shape, calls at the
    reference's batch sizes (--batch_size 2, scripts/search.sh:29; 128, src/arguments.py:60) make no hipMalloc — and
    give the same answer every time."""
    from mllm_sparse_retrieval_amd.dense import DenseIndex

    rng = np.random.default_rng(2)
    p, q = _unit_rows(rng, 9000, 64), _unit_rows(rng, 128, 64)
    dix = DenseIndex(p)
    first = {}
    for bs in (2, 128):
        first[bs] = dix.search(q[:bs], 100)
    base = dix.stats()["device_allocs"]
    assert base > 0
    for _ in range(5):
        for bs in (2, 128):
            s, i = dix.search(q[:bs], 100)
            assert (s == first[bs][0]).all() and (i == first[bs][1]).all()
    assert dix.stats()["device_allocs"] == base
    ws, wi = _dense_oracle(q, p, 100)
    assert np.abs(first[128][0] - ws).max() <= 1e-5
    dix.close()


def test_dense_gemm_random_shapes(m):
    """The four-wave GEMM kernel (grids of >= 256 blocks of 256 x 256) on random shapes: ragged last blocks in both
    directions, 1-8 steps of 64 in K, doc counts that are not multiples of 4; scores within 1e-5 of numpy on the
    fp16-rounded inputs, ranks equal except inside accumulation-noise ties. (MSR_FUZZ_SEED / MSR_FUZZ_CASES as above.)"""
    from mllm_sparse_retrieval_amd.dense import FaissFlatSearcher

    rng = np.random.default_rng(int(os.environ.get("MSR_FUZZ_SEED", "7")))
    for case in range(int(os.environ.get("MSR_FUZZ_CASES", "4"))):
        h = 64 * int(rng.integers(1, 9))
        n = int(rng.integers(4100, 7000))
        nq = int(rng.integers(max(4100, (256 * 256 * 256) // ((n + 255) // 256 * 256) + 1), 7000))
        k = int(rng.choice([1, 10, 100]))
        assert ((n + 255) // 256) * ((nq + 255) // 256) >= 256
        p, q = _unit_rows(rng, n, h), _unit_rows(rng, nq, h)
        r = FaissFlatSearcher(p)
        r.add(p)
        scores, idx = r.batch_search(q, k, batch_size=nq, quiet=True)         # ONE call: the grid is the whole product
        ws, wi = _dense_oracle(q, p, k)
        assert np.abs(scores - ws).max() <= 1e-5, (case, n, h, nq, k)
        diff = idx != wi
        if diff.any():
            exact = q.astype(np.float16).astype(np.float32) @ p.astype(np.float16).astype(np.float32).T
            gap = np.abs(ws - np.take_along_axis(exact, idx, axis=1))
            assert gap[diff].max() <= 2e-6 and diff.mean() < 0.01, (case, n, h, nq, k)
        del r


def test_hybrid_fusion_end_to_end(m, tmp_path):
    """Config-5 shape in small: sparse top-depth + dense top-depth -> get_run_dict -> fuse, against the same pipeline
    driven by the oracles (sparse: C port; dense: numpy on fp16-rounded inputs). Fused scores within 1e-5."""
    from types import SimpleNamespace

    from mllm_sparse_retrieval_amd.compat import FaissFlatSearcher, fuse, get_run_dict, search_queries
    from oracle import oracle

    n, nq, depth, n_terms, h = 3000, 100, 200, 2000, 128
    docs, (qp, qt, qw) = helpers.synth(n, 64, nq, 40, n_terms, seed=55)
    ids = [str(10000 + i) for i in range(n)]
    path = m.build_index_from_csr(str(tmp_path / "h.idx"), *docs, n_terms, doc_ids=ids)
    rng = np.random.default_rng(5)
    p, q = _unit_rows(rng, n, h), _unit_rows(rng, nq, h)
    qids = [str(i) for i in range(nq)]
    with m.SparseIndex(path, device=0) as ix:
        o, f, _, cnt = ix.search_csr(qp, qt, qw, depth)
        s_scores = [[float(x) for x in f[i, :cnt[i]]] for i in range(nq)]
        s_rank = [ix.docids(o[i, :cnt[i]]) for i in range(nq)]
    sparse_run = get_run_dict(qids, s_scores, s_rank, False)
    dr = FaissFlatSearcher(p)
    dr.add(p)
    d_scores, d_ids = search_queries(dr, q, ids, SimpleNamespace(batch_size=64, depth=depth, quiet=True))
    dense_run = get_run_dict(qids, d_scores, d_ids, False)
    fused = fuse([dense_run, sparse_run], [0.5, 0.5])
    # oracle pipeline
    oix, order = helpers.taat_oracle(docs, n_terms, ids)
    wo, ws, wn = oix.search(qp, qt, qw, depth, threads=8)
    sorted_ids = [ids[r] for r in order]
    o_sparse = oracle.get_run_dict(qids, [[float(np.float32(x)) for x in ws[i, :wn[i]]] for i in range(nq)],
                                   [[sorted_ids[int(d)] for d in wo[i, :wn[i]]] for i in range(nq)], False)
    dsc, didx = _dense_oracle(q, p, depth)
    o_dense = oracle.get_run_dict(qids, dsc, np.array([[ids[j] for j in row] for row in didx]), False)
    want = oracle.fuse([o_dense, o_sparse], [0.5, 0.5])
    worst = 0.0
    for qid in qids:
        common = set(fused[qid]) & set(want[qid])
        assert len(common) >= 0.99 * len(want[qid])          # fp16-tie neighbours at the depth boundary may differ
        worst = max(worst, max(abs(float(fused[qid][d]) - float(want[qid][d])) for d in common))
    assert worst <= 1e-5


@pytest.mark.parametrize("n,alpha,remove", [(3000, 0.5, False), (9000, 0.3, True)])
def test_gpu_fusion_matches_host_fuse(m, tmp_path, n, alpha, remove):
    """msr_hybrid_search (everything on the GPU) against the reference-semantics host pipeline
    get_run_dict + fuse (pinned to src/hybrid.py) fed with the same GPU lists: top-10 ids and fused scores (1e-5)."""
    from types import SimpleNamespace

    from mllm_sparse_retrieval_amd.compat import FaissFlatSearcher, fuse, get_run_dict, search_queries
    from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_search, row_to_ordinal

    nq, depth, n_terms, h, k = 120, 300, 2000, 64, 10
    docs, (qp, qt, qw) = helpers.synth(n, 64, nq, 40, n_terms, seed=n)
    ids = [str(i) for i in range(n)]
    path = m.build_index_from_csr(str(tmp_path / "f.idx"), *docs, n_terms, doc_ids=ids)
    rng = np.random.default_rng(n)
    p, q = _unit_rows(rng, n, h), _unit_rows(rng, nq, h)
    qids = [str(i) for i in range(nq)]                        # query ids collide with doc ids -> remove_query matters
    with m.SparseIndex(path, device=0) as ix:
        dix = DenseIndex(p)
        r2o = row_to_ordinal(ix, ids)
        self_ord = np.array([int(r2o[int(x)]) for x in qids], dtype=np.int32) if remove else None
        ords, fs, cnt, ms = hybrid_search(ix, dix, qp, qt, qw, q, depth, k, alpha, r2o, self_ord)
        got_ids = [ix.docids(ords[i, :cnt[i]]) for i in range(nq)]
        o, f, _, c = ix.search_csr(qp, qt, qw, depth)
        sparse_run = get_run_dict(qids, [[float(x) for x in f[i, :c[i]]] for i in range(nq)],
                                  [ix.docids(o[i, :c[i]]) for i in range(nq)], remove)
        dix.close()
    dr = FaissFlatSearcher(p)
    dr.add(p)
    d_scores, d_ids = search_queries(dr, q, ids, SimpleNamespace(batch_size=64, depth=depth, quiet=True))
    dense_run = get_run_dict(qids, d_scores, d_ids, remove)
    want = fuse([dense_run, sparse_run], [alpha, 1 - alpha])
    assert ms["sparse"] > 0 and ms["dense_gemm"] > 0  # (3 000 docs = one tile: fused kernel; 9 000 = list-based path)
    assert (ms["fusion"] > 0) == (n > 8192)
    for i, qid in enumerate(qids):
        ranked = sorted(want[qid].items(), key=lambda kv: (-float(kv[1]), kv[0].encode()))[:k]
        assert cnt[i] == len(ranked)
        for j, (doc, score) in enumerate(ranked):
            assert abs(float(fs[i, j]) - float(score)) <= 1e-5
            if got_ids[i][j] != doc:   # only a near-tie in the fused score may swap neighbours
                assert abs(float(want[qid][got_ids[i][j]]) - float(score)) <= 2e-6
        if remove:
            assert qid not in got_ids[i]


def test_c5_real_shape_dense_and_hybrid_vs_oracle_pipeline(m, tmp_path):
    """BASELINE config 5 at its REAL shape (scripts/search.sh:25,32): N = 5 000 docs x (128 nnz + 4096-d fp16), 25 010
    queries x (120 nnz + 4096-d), depth 1000 -> fused top-10, alpha 0.5. All queries run on the GPU (the 256 x 256
    LDS-DMA GEMM instance, K = 4096 accumulation); a sample of every 25th query is checked against
      (a) dense: numpy f32 inner products of the fp16-rounded inputs, top-1000, scores within 1e-5,
      (b) hybrid: the ORACLE pipeline — C oracle sparse top-1000 + numpy dense top-1000 -> oracle.get_run_dict ->
          oracle.fuse (pinned to src/hybrid.py:32-53) -> top-10 — fused scores within 1e-5, ids equal up to near-ties."""
    from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_search, row_to_ordinal
    from oracle import oracle

    n, nq, h, depth, k, alpha, n_terms = 5000, 25010, 4096, 1000, 10, 0.5, 30000
    docs = m.synth_vectors(n, 128, n_terms, seed=4, threads=16)
    qp, qt, qw = m.synth_vectors(nq, 120, n_terms, seed=5, threads=16)
    qp, qt, qw = qp.astype(np.int64), qt.astype(np.int32), qw.astype(np.int32)
    rng = np.random.default_rng(4)
    p, q = _unit_rows(rng, n, h), _unit_rows(rng, nq, h)
    ids = [str(i) for i in range(n)]
    path = m.build_index_from_csr(str(tmp_path / "c5.idx"), *docs, n_terms, doc_ids=ids)
    sample = np.arange(0, nq, 25)
    with m.SparseIndex(path, device=0) as ix:
        dix = DenseIndex(p)
        d_scores, d_idx = dix.search(q, depth)
        r2o = row_to_ordinal(ix, ids)
        ords, fs, cnt, ms = hybrid_search(ix, dix, qp, qt, qw, q, depth, k, alpha, r2o)
        got_ids = {int(i): ix.docids(ords[i, :cnt[i]]) for i in sample}
        dix.close()
    assert ms["dense_gemm"] > 0 and ms["sparse"] > 0 and ms["fusion"] == 0   # one tile: the fused kernel
    # (a) dense top-1000 of the sampled queries
    ws, wi = _dense_oracle(q[sample], p, depth)
    assert np.abs(d_scores[sample] - ws).max() <= 1e-5
    diff = d_idx[sample] != wi
    if diff.any():  # rows may swap only where two scores are closer than the f32 accumulation noise
        s_all = q[sample].astype(np.float16).astype(np.float32) @ p.astype(np.float16).astype(np.float32).T
        gap = np.abs(ws - np.take_along_axis(s_all, d_idx[sample], axis=1))
        assert gap[diff].max() <= 2e-6 and diff.mean() < 0.01
    assert (np.diff(d_scores, axis=1) <= 0).all() and (d_idx >= 0).all()
    # (b) the oracle pipeline on the sampled queries
    oix, order = helpers.taat_oracle(docs, n_terms, ids)
    sorted_ids = [ids[r] for r in order]
    sel = np.concatenate([np.arange(qp[i], qp[i + 1]) for i in sample])
    sp = np.concatenate([[0], np.cumsum(qp[sample + 1] - qp[sample])]).astype(np.int64)
    wo, wsc, wn = oix.search(sp, qt[sel], qw[sel], depth, threads=16)
    qids = [str(int(i)) for i in sample]
    o_sparse = oracle.get_run_dict(qids, [[float(np.float32(x)) for x in wsc[j, :wn[j]]] for j in range(len(sample))],
                                   [[sorted_ids[int(d)] for d in wo[j, :wn[j]]] for j in range(len(sample))], False)
    o_dense = oracle.get_run_dict(qids, ws, np.array([[ids[j] for j in row] for row in wi]), False)
    want = oracle.fuse([o_dense, o_sparse], [alpha, 1 - alpha])
    worst = 0.0
    for j, i in enumerate(sample):
        qid = qids[j]
        ranked = sorted(want[qid].items(), key=lambda kv: (-float(kv[1]), kv[0].encode()))[:k]
        assert cnt[i] == len(ranked) == k
        for r, (doc, score) in enumerate(ranked):
            worst = max(worst, abs(float(fs[i, r]) - float(score)))
            g = got_ids[int(i)][r]
            if g != doc:  # only a near-tie in the fused score may swap neighbours
                assert g in want[qid] and abs(float(want[qid][g]) - float(score)) <= 2e-6, (qid, r, g, doc)
    assert worst <= 1e-5


@pytest.mark.parametrize("n,tile,depth,k,alpha,remove", [(3000, 0, 300, 10, 0.5, False), (3000, 0, 100, 10, 0.3, True),
                                                       (8000, 0, 1000, 64, 0.7, False), (700, 4096, 1024, 10, 0.5, False),
                                                       (5000, 0, 5000 // 5, 1, 0.0, False), (4097, 8192, 50, 5, 1.0, True)])
def test_fused_hybrid_tile_vs_oracle_pipeline(m, tmp_path, n, tile, depth, k, alpha, remove):
    """The fused single-tile hybrid kernel (scores + both depth-selections + fusion + top-k in one workgroup per query)
    against the oracle pipeline, every query: list sizes above and below the corpus size, alpha at both ends (one run
    contributes nothing but still defines membership of the union), remove_query, k = 1 and k = 64."""
    from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_search, row_to_ordinal

    nq, n_terms, h = 150, 2000, 64
    docs, (qp, qt, qw) = helpers.synth(n, 48, nq, 30, n_terms, seed=n + depth)
    ids = [str(i) for i in range(n)]
    path = m.build_index_from_csr(str(tmp_path / "f.idx"), *docs, n_terms, doc_ids=ids, tile_docs=tile)
    rng = np.random.default_rng(n)
    p, q = _unit_rows(rng, n, h), _unit_rows(rng, nq, h)
    qids = [str(i) for i in range(nq)]                        # query ids collide with doc ids -> remove_query matters
    with m.SparseIndex(path, device=0) as ix:
        assert ix.n_tiles == 1
        dix = DenseIndex(p)
        r2o = row_to_ordinal(ix, ids)
        self_ord = np.array([int(r2o[int(x)]) for x in qids], dtype=np.int32) if remove else None
        ords, fs, cnt, ms = hybrid_search(ix, dix, qp, qt, qw, q, min(depth, 1024), k, alpha, r2o, self_ord)
        assert ms["dense_select"] == 0 and ms["fusion"] == 0 and ms["sparse"] > 0   # the fused kernel ran
        docid_of = ix.docid
        sample = np.arange(nq)
        want, sq = helpers.oracle_hybrid(docs, n_terms, ids, qp, qt, qw, q, p, min(depth, 1024), alpha, sample, remove, qids)
        helpers.assert_hybrid_matches(want, sq, sample, ords, fs, cnt, docid_of, k)
        if remove:
            assert all(qids[i] not in [docid_of(int(o)) for o in ords[i, :cnt[i]]] for i in range(nq))
        dix.close()


def test_fused_hybrid_randomised(m, tmp_path):
    """Fuzz of the fused hybrid kernel against the oracle pipeline: corpus sizes on both sides of the tile / round
    boundaries, depths from 1 to 1024, k from 1 to 64, alpha incl. 0 and 1, remove_query, short and empty queries
    (docs with score 0 on the sparse side), small vocabularies (many sparse ties), dense dims 32-160, duplicated passage
    rows (exact dense ties: ids may differ inside a tie, scores may not)."""
    from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_search, row_to_ordinal

    rng = np.random.default_rng(int(os.environ.get("MSR_FUZZ_SEED", "20251005")))
    for case in range(int(os.environ.get("MSR_FUZZ_CASES", "14"))):
        n = int(rng.choice([37, 700, 2047, 2049, 4096, 4097, 6000, 8192]))
        n_terms = int(rng.choice([6, 60, 2000]))
        nnz = int(min(n_terms, rng.integers(1, 24)))
        nq = min(int(rng.integers(3, 40)), n)                               # (query ids are doc ids: keep them distinct)
        qn = int(min(n_terms, rng.integers(0, 12)))
        depth = int(rng.choice([1, 7, 100, 1000, 1024]))
        k = int(rng.choice([1, 10, 64]))
        alpha = float(rng.choice([0.0, 0.3, 0.5, 1.0]))
        remove = bool(rng.integers(0, 2))
        h = int(rng.choice([32, 64, 160]))
        dp = np.arange(0, n * nnz + 1, nnz, dtype=np.uint64)
        dt = np.concatenate([rng.choice(n_terms, nnz, replace=False) for _ in range(n)]).astype(np.uint32)
        dw = rng.integers(1, 300, n * nnz).astype(np.uint32)
        qp = np.arange(nq + 1, dtype=np.int64) * qn                         # (qn may be 0: empty queries)
        qt = rng.integers(0, n_terms, nq * qn).astype(np.int32)
        qw = rng.integers(0, 50, nq * qn).astype(np.int32)
        ids = [str(int(x)) for x in rng.permutation(n * 3)[:n]]            # ids in no particular order
        path = m.build_index_from_csr(str(tmp_path / f"z{case}.idx"), dp, dt, dw, n_terms, doc_ids=ids)
        p = _unit_rows(rng, n, h)
        if case % 3 == 0:
            p[1::2] = p[0::2][: len(p[1::2])]                               # every passage row twice: exact dense ties
        q = _unit_rows(rng, nq, h)
        qids = [ids[int(i) % n] for i in range(nq)]                          # query ids that ARE doc ids (remove_query)
        with m.SparseIndex(path, device=0) as ix:
            assert ix.n_tiles == 1
            dix = DenseIndex(p)
            r2o = row_to_ordinal(ix, ids)
            self_ord = np.array([int(r2o[int(i) % n]) for i in range(nq)], dtype=np.int32) if remove else None
            ords, fs, cnt, ms = hybrid_search(ix, dix, qp, qt, qw, q, depth, k, alpha, r2o, self_ord)
            assert ms["fusion"] == 0 and ms["dense_select"] == 0
            docid_of = ix.docid
            # (exact dense ties — the duplicated rows — go to the lower doc ORDINAL in the fused kernel, to the lower row
            # in the reference's flat index: the oracle is told the kernel's rule, so that the depth boundary cuts the
            # same twin on both sides)
            want, sq = helpers.oracle_hybrid((dp, dt, dw), n_terms, ids, qp, qt, qw, q, p, depth, alpha, np.arange(nq),
                                             remove, qids, dense_tie_key=r2o)
            # min-max normalisation divides by the spread of the top-depth list: the f32 accumulation-order noise of the
            # raw dense scores (a few 1e-7 at these dimensions; the 1e-5 of the north star is the bound on RAW scores)
            # reaches the fused score multiplied by alpha / spread — a small depth on a large corpus has a small spread
            dsc_o, _ = helpers.dense_oracle(q, p, min(depth, n), r2o)
            spread = np.maximum(dsc_o[:, 0] - dsc_o[:, -1], 1e-3)
            for i in range(nq):
                tol = 1e-5 + alpha * 1e-6 / float(spread[i])
                ranked = sorted(want[sq[i]].items(), key=lambda kv: (-float(kv[1]), kv[0].encode()))[:k]
                assert cnt[i] == len(ranked), (case, i, cnt[i], len(ranked))
                got = [docid_of(int(o)) for o in ords[i, : cnt[i]]]
                assert len(set(got)) == len(got)
                for r, (doc, score) in enumerate(ranked):
                    # scores position by position (a dense tie at the depth boundary may admit the twin row instead:
                    # the same score then sits on another id)
                    assert abs(float(fs[i, r]) - float(score)) <= tol, (case, i, r, float(fs[i, r]), float(score), tol)
                if remove:
                    assert qids[i] not in got
            dix.close()
        os.remove(path)


def _hybrid_case(m, tmp_path, n, tile, nq, depth, k, alpha, remove, h=64, n_terms=2000, seed=0, doc_nnz=48, q_nnz=30,
                 expect="multi"):
    """One corpus through msr_hybrid_search against the oracle pipeline, every query."""
    from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_search, row_to_ordinal

    docs, (qp, qt, qw) = helpers.synth(n, doc_nnz, nq, q_nnz, n_terms, seed=seed or (n + depth))
    rng = np.random.default_rng(n + 7)
    ids = [str(int(x)) for x in rng.permutation(3 * n)[:n]]       # ids in no particular order: ordinals != rows
    path = m.build_index_from_csr(str(tmp_path / "mt.idx"), *docs, n_terms, doc_ids=ids, tile_docs=tile)
    p, q = _unit_rows(rng, n, h), _unit_rows(rng, nq, h)
    qids = [ids[i] for i in range(nq)]                             # query ids that ARE doc ids (remove_query matters)
    with m.SparseIndex(path, device=0) as ix:
        dix = DenseIndex(p)
        r2o = row_to_ordinal(ix, ids)
        self_ord = np.array([int(r2o[i]) for i in range(nq)], dtype=np.int32) if remove else None
        ords, fs, cnt, ms = hybrid_search(ix, dix, qp, qt, qw, q, depth, k, alpha, r2o, self_ord)
        if expect == "multi":   # hybrid_tiles<MODE 1> + hybrid_fuse_query: {candidates, GEMM, 0, fusion}
            assert ms["sparse"] > 0 and ms["dense_gemm"] > 0 and ms["dense_select"] == 0 and ms["fusion"] > 0
        want, sq = helpers.oracle_hybrid(docs, n_terms, ids, qp, qt, qw, q, p, depth, alpha, np.arange(nq), remove, qids,
                                         dense_tie_key=r2o)
        helpers.assert_hybrid_matches(want, sq, np.arange(nq), ords, fs, cnt, ix.docid, k)
        if remove:
            assert all(qids[i] not in [ix.docid(int(o)) for o in ords[i, :cnt[i]]] for i in range(nq))
        n_tiles = ix.n_tiles
        dix.close()
    return n_tiles


@pytest.mark.parametrize("n,tile,depth,k,alpha,remove", [(9000, 0, 300, 10, 0.5, False), (20000, 4096, 1000, 64, 0.3, True),
                                                       (25010, 0, 1000, 200, 0.5, True), (8200, 8192, 1024, 1024, 0.7, False),
                                                       (12000, 4096, 50, 1, 0.0, True), (16385, 8192, 7, 5, 1.0, False),
                                                       (5000, 0, 1000, 200, 0.5, True)])
def test_multitile_hybrid_vs_oracle_pipeline(m, tmp_path, n, tile, depth, k, alpha, remove):
    """Multi-tile indexes (and k > 64 on one tile) through the candidate kernels: hybrid_tiles<MODE 1> emits every tile's
    quota of candidates per side, hybrid_fuse_query finds both depth-th bests, fuses and ranks. Against the oracle pipeline
    (C oracle sparse + numpy dense -> oracle.get_run_dict -> oracle.fuse, pinned to src/hybrid.py:32-53), every query:
    the reference's own hybrid shape in small (25 010 docs, depth 1000, remove_query, scripts/search.sh:25-27), the
    recall reporter's k = 200 (src/metrices.py:9), k = depth = 1024, a last tile of one doc, alpha at both ends."""
    tiles = _hybrid_case(m, tmp_path, n, tile, 60, depth, k, alpha, remove)
    assert tiles == (n + (tile or 8192) - 1) // (tile or 8192)


def test_multitile_hybrid_edges(m, tmp_path):
    """The candidate kernels at the edges: no queries at all, a corpus of one / three docs (k > 64 sends even a single tile
    down this path), depth and k larger than the corpus, every query empty on the sparse side."""
    from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_search, row_to_ordinal

    for n in (1, 3, 4097):
        tiles = _hybrid_case(m, tmp_path, n, 4096, min(n, 8), 1024, 100, 0.5, n > 1, n_terms=50, doc_nnz=min(5, 50),
                             q_nnz=3, expect="multi")
        assert tiles == (n + 4095) // 4096
    docs, (qp, qt, qw) = helpers.synth(9000, 16, 6, 4, 300, seed=5)
    path = m.build_index_from_csr(str(tmp_path / "e.idx"), *docs, 300, tile_docs=4096)
    rng = np.random.default_rng(1)
    p, q = _unit_rows(rng, 9000, 32), _unit_rows(rng, 6, 32)
    with m.SparseIndex(path, device=0) as ix:
        dix = DenseIndex(p)
        r2o = row_to_ordinal(ix, [str(i) for i in range(9000)])
        # no queries
        o, f, c, ms = hybrid_search(ix, dix, np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32),
                                    np.zeros((0, 32), np.float32), 100, 10, 0.5, r2o)
        assert o.shape == (0, 10) and c.shape == (0,)
        # queries without a single sparse term: the union is the dense depth list alone
        o, f, c, ms = hybrid_search(ix, dix, np.zeros(7, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32), q, 50, 64,
                                    0.5, r2o)
        assert (c == 50).all() and ms["fusion"] > 0
        sfull = q.astype(np.float16).astype(np.float32) @ p.astype(np.float16).astype(np.float32).T
        for i in range(6):
            top = np.argsort(-sfull[i], kind="stable")[:50]
            assert set(int(r2o[r]) for r in top) == set(int(x) for x in o[i, :50])
            assert abs(float(f[i, 0]) - 0.5) <= 1e-6 and float(f[i, 49]) == 0.0   # min-max: best = alpha, the 50th = 0
        dix.close()


def test_multitile_hybrid_second_round(m, tmp_path, monkeypatch):
    """A quota too small for the depth lists (forced through MSR_HYBRID_QUOTA): hybrid_fuse_query flags every query and
    the second round (every tile emits its own top-depth) produces the same exact result; and sparse lists that live in
    ONE tile (the queries' terms occur only in the first 300 ordinals), which no share-based quota covers."""
    monkeypatch.setenv("MSR_HYBRID_QUOTA", "3")
    _hybrid_case(m, tmp_path, 20000, 4096, 40, 400, 10, 0.5, True)
    monkeypatch.delenv("MSR_HYBRID_QUOTA")
    from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_search, row_to_ordinal

    n, nq, n_terms, h, depth, k = 18000, 30, 500, 32, 250, 10
    rng = np.random.default_rng(5)
    # docs 0 .. 299 (ids "00000" .. = the lowest ordinals: one tile) hold terms 0-99, all other docs terms 100-499
    nnz = 20
    dp = np.arange(0, n * nnz + 1, nnz, dtype=np.uint64)
    dt = np.concatenate([rng.choice(100, nnz, replace=False) if i < 300 else 100 + rng.choice(400, nnz, replace=False)
                         for i in range(n)]).astype(np.uint32)
    dw = rng.integers(1, 300, n * nnz).astype(np.uint32)
    ids = [f"{i:05d}" for i in range(n)]
    qp = np.arange(nq + 1, dtype=np.int64) * 10
    qt = rng.integers(0, 100, nq * 10).astype(np.int32)
    qw = rng.integers(1, 50, nq * 10).astype(np.int32)
    path = m.build_index_from_csr(str(tmp_path / "one.idx"), dp, dt, dw, n_terms, doc_ids=ids, tile_docs=4096)
    p, q = _unit_rows(rng, n, h), _unit_rows(rng, nq, h)
    with m.SparseIndex(path, device=0) as ix:
        dix = DenseIndex(p)
        r2o = row_to_ordinal(ix, ids)
        ords, fs, cnt, ms = hybrid_search(ix, dix, qp, qt, qw, q, depth, k, 0.5, r2o)
        want, sq = helpers.oracle_hybrid((dp, dt, dw), n_terms, ids, qp, qt, qw, q, p, depth, 0.5, np.arange(nq),
                                         dense_tie_key=r2o)
        helpers.assert_hybrid_matches(want, sq, np.arange(nq), ords, fs, cnt, ix.docid, k)
        dix.close()


def test_hybrid_reference_shape_i2t_full(m, tmp_path):
    """The reference's OWN hybrid run at its real shape (scripts/search.sh:5,16-33: TARGET_TYPE=text, --query_type
    image, --depth 1000, --remove_query, --alpha 0.5; COCO-5K test split): 5 000 image queries over 25 010 caption docs,
    H = 4096, fused top-10. All queries run on the GPU; every 25th is checked against the oracle pipeline (ids equal up
    to 2e-6 near-ties, fused scores within 1e-5) — once through the candidate kernels and once through the list-based
    path (score_tiles / select_tiles / fuse_tiles), which has to give the same answer."""
    import subprocess
    import sys

    from mllm_sparse_retrieval_amd import workloads
    from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_search, row_to_ordinal

    n, nq, h, depth, k, alpha, n_terms = 25010, 5000, 4096, 1000, 10, 0.5, 30000
    docs, (qp, qt, qw), p, q = workloads.hybrid_vectors(n, nq, h)
    ids = [str(i) for i in range(n)]
    path = m.build_index_from_csr(str(tmp_path / "i2t.idx"), *docs, n_terms, doc_ids=ids)
    sample = np.arange(0, nq, 25)
    qids = [str(i) for i in range(nq)]                          # image ids collide with caption ids: remove_query acts
    with m.SparseIndex(path, device=0) as ix:
        assert ix.n_tiles == 4
        dix = DenseIndex(p)
        r2o = row_to_ordinal(ix, ids)
        self_ord = r2o[:nq].astype(np.int32)
        ords, fs, cnt, ms = hybrid_search(ix, dix, qp, qt, qw, q, depth, k, alpha, r2o, self_ord)
        assert ms["dense_select"] == 0 and ms["fusion"] > 0   # the candidate kernels ran
        want, sq = helpers.oracle_hybrid(docs, n_terms, ids, qp, qt, qw, q, p, depth, alpha, sample, True, qids,
                                         dense_tie_key=r2o)
        helpers.assert_hybrid_matches(want, sq, sample, ords, fs, cnt, ix.docid, k)
        assert all(qids[i] not in [ix.docid(int(o)) for o in ords[i, :cnt[i]]] for i in sample)
        dix.close()
    np.savez(tmp_path / "got.npz", ords=ords, fs=fs, cnt=cnt)
    # the list-based path in a child process (the switch is read once per process)
    code = f"""
import sys, numpy as np
sys.path.insert(0, {os.path.dirname(os.path.dirname(os.path.abspath(__file__)))!r})
import mllm_sparse_retrieval_amd as m
from mllm_sparse_retrieval_amd import workloads
from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_search, row_to_ordinal
docs, (qp, qt, qw), p, q = workloads.hybrid_vectors({n}, {nq}, {h})
with m.SparseIndex({path!r}, device=0) as ix:
    dix = DenseIndex(p)
    r2o = row_to_ordinal(ix, [str(i) for i in range({n})])
    ords, fs, cnt, ms = hybrid_search(ix, dix, qp, qt, qw, q, {depth}, {k}, {alpha}, r2o, r2o[:{nq}].astype(np.int32))
    assert ms["dense_select"] > 0, ms
    dix.close()
np.savez({str(tmp_path / "list.npz")!r}, ords=ords, fs=fs, cnt=cnt)
"""
    subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, MSR_NO_FUSED_HYBRID="1"))
    lst = np.load(tmp_path / "list.npz")
    with m.SparseIndex(path, device=-1) as ixh:
        helpers.assert_hybrid_matches(want, sq, sample, lst["ords"], lst["fs"], lst["cnt"], ixh.docid, k)
    # the two paths agree on every query up to near-ties (dense ties at the depth boundary: ordinal vs row rule)
    same = (lst["ords"] == ords).all(axis=1)
    assert same.mean() > 0.99 and np.abs(lst["fs"] - fs).max() <= 1e-5


def test_fused_hybrid_tightly_clustered_scores(m, tmp_path):
    """Scores far from 0 with a tiny spread (round 2's advisor finding: a histogram offset rounded in f32 put the top bin
    past the array): sparse scores 2e7 + [1, 300] (one heavy term almost every doc holds), and dense scores
    138.5 + j * 2^-16 for j in 0..3 (exactly representable: ties in blocks, cut by ordinal). Each side is checked through
    a list only IT fills: an empty sparse query (union = the dense depth list) and alpha = 0 with depth-limited sparse."""
    from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_search, row_to_ordinal

    n, V, h, nq, depth, k = 3000, 50, 32, 24, 50, 64
    rng = np.random.default_rng(9)
    # every doc but the last holds term 0 with weight 40 000; every doc holds one light term 1 .. 49 with weight 1 .. 300
    dp = np.concatenate([np.arange(0, 2 * (n - 1) + 1, 2), [2 * (n - 1) + 1]]).astype(np.uint64)
    dt = np.concatenate([np.stack([np.zeros(n - 1, np.uint32), rng.integers(1, V, n - 1).astype(np.uint32)], 1).ravel(),
                         [1]]).astype(np.uint32)
    dw = np.concatenate([np.stack([np.full(n - 1, 40000, np.uint32), rng.integers(1, 301, n - 1).astype(np.uint32)], 1).ravel(),
                         [5]]).astype(np.uint32)
    ids = [str(i) for i in range(n)]
    path = m.build_index_from_csr(str(tmp_path / "cl.idx"), dp, dt, dw, V, doc_ids=ids)
    # queries 0-11: term 0 x 500 + every light term x 1 (scores 2e7 + light weight); queries 12-23: empty
    qterms = np.concatenate([[0], np.arange(1, V)]).astype(np.int32)
    qweights = np.concatenate([[500], np.ones(V - 1)]).astype(np.int32)
    qp = np.concatenate([np.arange(13) * V, np.full(12, 12 * V)]).astype(np.int64)
    qt, qw = np.tile(qterms, 12), np.tile(qweights, 12)
    p = np.zeros((n, h), np.float32)
    p[:, 0] = 1.0
    p[:, 1] = (np.arange(n) % 4) * 2.0 ** -10
    q = np.zeros((nq, h), np.float32)
    q[:, 0] = 138.5
    q[:, 1] = 2.0 ** -6
    with m.SparseIndex(path, device=0) as ix:
        dix = DenseIndex(p)
        r2o = row_to_ordinal(ix, ids)
        for alpha in (0.0, 1.0, 0.5):
            ords, fs, cnt, ms = hybrid_search(ix, dix, qp, qt, qw, q, depth, k, alpha, r2o)
            want, sq = helpers.oracle_hybrid((dp, dt, dw), V, ids, qp, qt, qw, q, p, depth, alpha, np.arange(nq),
                                             dense_tie_key=r2o)
            # the union of two depth-50 lists: at most 100 docs, exactly 50 for the empty queries — a threshold that came
            # out too low would fill all 64 places
            assert (cnt[12:] == depth).all()
            helpers.assert_hybrid_matches(want, sq, np.arange(nq), ords, fs, cnt, ix.docid, k)
        dix.close()


def test_multitile_hybrid_randomised(m, tmp_path, monkeypatch):
    """Fuzz of the candidate kernels (hybrid_tiles<MODE 1> + hybrid_fuse_query) against the oracle pipeline: 2-5 tiles of
    4096 or 8192 docs incl. a last tile of one doc, depths 1-1024, k 1-1024, alpha incl. 0 and 1, remove_query, empty and
    short queries, small vocabularies (mass ties on the sparse side), duplicated passage rows (exact dense ties), and — every
    third case — a forced quota of 1-40 candidates per tile, so that hybrid_fuse_query's verification has to send queries
    to the second round. (MSR_FUZZ_SEED / MSR_FUZZ_CASES as in the other fuzz tests.) One msr_hybrid_search_union call per
    case pins what the tolerances above leave open: its fused bits and its order follow exactly from its own side arrays
    (helpers.assert_union_arithmetic), and the top-k call returns its first k ordinals and score bits."""
    from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_search, hybrid_search_union, row_to_ordinal

    rng = np.random.default_rng(int(os.environ.get("MSR_FUZZ_SEED", "20261005")))
    for case in range(int(os.environ.get("MSR_FUZZ_CASES", "12"))):
        tile = int(rng.choice([4096, 8192]))
        n = int(rng.choice([tile + 1, tile + 700, 2 * tile, 2 * tile + 1, 3 * tile - 5, 4 * tile + 33]))
        n_terms = int(rng.choice([6, 60, 2000]))
        nnz = int(min(n_terms, rng.integers(1, 20)))
        nq = int(rng.integers(3, 24))
        qn = int(min(n_terms, rng.integers(0, 12)))
        depth = int(rng.choice([1, 7, 100, 1000, 1024]))
        k = int(rng.choice([1, 10, 64, 200, 1024]))
        alpha = float(rng.choice([0.0, 0.3, 0.5, 1.0]))
        remove = bool(rng.integers(0, 2))
        h = int(rng.choice([32, 64]))
        if case % 3 == 2:
            monkeypatch.setenv("MSR_HYBRID_QUOTA", str(int(rng.integers(1, 41))))
        else:
            monkeypatch.delenv("MSR_HYBRID_QUOTA", raising=False)
        dp = np.arange(0, n * nnz + 1, nnz, dtype=np.uint64)
        dt = (rng.integers(0, n_terms, (n, 1)) + np.arange(nnz)[None, :] * max(n_terms // max(nnz, 1), 1)) % n_terms
        dt = np.sort(dt, axis=1)
        if nnz > 1 and (np.diff(dt, axis=1) == 0).any():   # (distinct terms per row)
            dt = np.stack([rng.choice(n_terms, nnz, replace=False) for _ in range(n)])
        dt = dt.astype(np.uint32).ravel()
        dw = rng.integers(1, 300, n * nnz).astype(np.uint32)
        qp = np.arange(nq + 1, dtype=np.int64) * qn
        qt = rng.integers(0, n_terms, nq * qn).astype(np.int32)
        qw = rng.integers(0, 50, nq * qn).astype(np.int32)
        ids = [str(int(x)) for x in rng.permutation(n * 3)[:n]]
        path = m.build_index_from_csr(str(tmp_path / f"mz{case}.idx"), dp, dt, dw, n_terms, doc_ids=ids, tile_docs=tile)
        p = _unit_rows(rng, n, h)
        if case % 4 == 0:
            p[1::2] = p[0::2][: len(p[1::2])]                               # every passage row twice: exact dense ties
        q = _unit_rows(rng, nq, h)
        qids = [ids[i] for i in range(nq)]
        with m.SparseIndex(path, device=0) as ix:
            assert ix.n_tiles == (n + tile - 1) // tile >= 2
            dix = DenseIndex(p)
            r2o = row_to_ordinal(ix, ids)
            self_ord = np.array([int(r2o[i]) for i in range(nq)], dtype=np.int32) if remove else None
            ords, fs, cnt, ms = hybrid_search(ix, dix, qp, qt, qw, q, depth, k, alpha, r2o, self_ord)
            assert ms["dense_select"] == 0 and ms["fusion"] > 0
            docid_of = ix.docid
            want, sq = helpers.oracle_hybrid((dp, dt, dw), n_terms, ids, qp, qt, qw, q, p, depth, alpha, np.arange(nq),
                                             remove, qids, dense_tie_key=r2o)
            dsc_o, _ = helpers.dense_oracle(q, p, min(depth, n), r2o)
            spread = np.maximum(dsc_o[:, 0] - dsc_o[:, -1], 1e-3)
            for i in range(nq):
                tol = 1e-5 + alpha * 1e-6 / float(spread[i])
                ranked = sorted(want[sq[i]].items(), key=lambda kv: (-float(kv[1]), kv[0].encode()))[:k]
                assert cnt[i] == len(ranked), (case, i, cnt[i], len(ranked))
                got = [docid_of(int(o)) for o in ords[i, : cnt[i]]]
                assert len(set(got)) == len(got)
                for r, (doc, score) in enumerate(ranked):
                    assert abs(float(fs[i, r]) - float(score)) <= tol, (case, i, r, float(fs[i, r]), float(score), tol)
                if remove:
                    assert qids[i] not in got
            un = hybrid_search_union(ix, dix, qp, qt, qw, q, depth, alpha, r2o, self_ord)
            helpers.assert_union_arithmetic(un, alpha)
            kk = min(k, 2 * depth)
            assert (cnt == np.minimum(un[2], k)).all(), case
            assert (ords[:, :kk] == un[0][:, :kk]).all() and (ords[:, kk:] == 0xFFFFFFFF).all(), case
            assert (fs.view(np.uint32)[:, :kk] == un[1].view(np.uint32)[:, :kk]).all(), case
            assert (fs.view(np.uint32)[:, kk:] == 0).all(), case
            dix.close()
        os.remove(path)
    monkeypatch.delenv("MSR_HYBRID_QUOTA", raising=False)


def test_fused_hybrid_mass_ties(m, tmp_path):
    """Every doc holds the same term with the same weight: all sparse scores tie, so the sparse top-`depth` list is the
    `depth` LOWEST ordinals (doc-id string order) — the selection's histogram collapses into one bin and has to split
    it by ordinal. Dense vectors repeat in blocks of 8, so dense scores tie exactly as well."""
    from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_search, row_to_ordinal

    n, V, h, nq, depth, k = 6000, 8, 32, 40, 700, 10
    dp = np.arange(n + 1, dtype=np.uint64)
    dt = np.full(n, 3, dtype=np.uint32)
    dw = np.full(n, 7, dtype=np.uint32)
    dt[::2] = 4
    ids = [str(i) for i in range(n)]
    path = m.build_index_from_csr(str(tmp_path / "t.idx"), dp, dt, dw, V, doc_ids=ids)
    qp = np.arange(nq + 1, dtype=np.int64)
    qt = np.where(np.arange(nq) % 2 == 0, 3, 4).astype(np.int32)
    qw = np.full(nq, 2, dtype=np.int32)
    rng = np.random.default_rng(1)
    base = _unit_rows(rng, n // 8, h)
    p = np.repeat(base, 8, axis=0)
    q = _unit_rows(rng, nq, h)
    with m.SparseIndex(path, device=0) as ix:
        dix = DenseIndex(p)
        r2o = row_to_ordinal(ix, ids)
        ords, fs, cnt, ms = hybrid_search(ix, dix, qp, qt, qw, q, depth, k, 0.5, r2o)
        # sparse side: the 700 lowest ordinals among the 3 000 docs that hold the query's term, all at normalised score
        # (s - min) / max(max - min, 1e-9) = 0 -> the fused score is the dense half alone, and a doc outside BOTH lists
        # cannot appear. Dense ties (8 equal rows) are cut by ordinal in the fused path: membership of the dense list
        # is checked through the score alone.
        sfull = q.astype(np.float16).astype(np.float32) @ p.astype(np.float16).astype(np.float32).T
        term_docs = {3: np.flatnonzero(dt == 3), 4: np.flatnonzero(dt == 4)}
        for i in range(nq):
            rows_with_term = term_docs[int(qt[i])]
            by_ord = sorted(rows_with_term, key=lambda r: r2o[r])[:depth]          # sparse list = lowest ordinals
            kth = np.sort(sfull[i])[::-1][depth - 1]
            dmin, dmax = kth, sfull[i].max()
            assert cnt[i] == k
            for j in range(k):
                row = int(np.flatnonzero(r2o == ords[i, j])[0])
                in_dense = sfull[i, row] >= kth - 1e-7
                assert in_dense or row in by_ord
                want = 0.5 * (sfull[i, row] - dmin) / max(dmax - dmin, 1e-9) if in_dense else 0.0
                assert abs(float(fs[i, j]) - want) <= 1e-5
            assert (np.diff(fs[i, :k]) <= 0).all()
        dix.close()


def test_randomised_configurations(m, tmp_path):
    """Fuzz: random corpus shapes, vocabularies, weights (including the 65 535 maximum), tile sizes, dense-head
    options, query shapes (OOV, zero weights, repeats) and k, each against the C oracle."""
    # (MSR_FUZZ_SEED / MSR_FUZZ_CASES: longer sessions with other seeds, scripts/gpu_fuzz.sh)
    rng = np.random.default_rng(int(os.environ.get("MSR_FUZZ_SEED", "20250418")))
    for case in range(int(os.environ.get("MSR_FUZZ_CASES", "24"))):
        n_docs = int(rng.integers(1, 20000))
        n_terms = int(rng.integers(1, 400))
        nnz = int(rng.integers(1, min(n_terms, 40) + 1))
        tile = int(rng.choice([4096, 8192, 12288, 16384, 32768]))
        dp = np.arange(0, n_docs * nnz + 1, nnz, dtype=np.uint64)
        if n_docs * nnz < 200000:
            dt = np.concatenate([rng.choice(n_terms, nnz, replace=False) for _ in range(n_docs)]).astype(np.uint32)
        else:
            dt = rng.integers(0, n_terms, n_docs * nnz).astype(np.uint32)
        hi = int(rng.choice([3, 50, 400, 65535]))
        dw = rng.integers(0, hi + 1, n_docs * nnz).astype(np.uint32)
        # repeated terms inside a row add up: keep the sum within the 16-bit weight range
        if hi == 65535:
            dw = np.minimum(dw, 65535 // nnz).astype(np.uint32)
        nq = int(rng.integers(1, 60))
        qn = int(rng.integers(1, 30))
        qp = np.arange(0, nq * qn + 1, qn, dtype=np.int64)
        qt = rng.integers(-1, n_terms, nq * qn).astype(np.int32)
        qw = rng.integers(-1, 40, nq * qn).astype(np.int32)
        m.set_build_option("dense_max_terms", int(rng.choice([0, 3, 16, 32])))
        m.set_build_option("dense_min_density", float(rng.choice([0.01, 0.2, 0.4, 0.9])))
        try:
            path = m.build_index_from_csr(str(tmp_path / f"z{case}.idx"), dp, dt, dw, n_terms, tile_docs=tile)
        finally:
            m.set_build_option("dense_max_terms", 16)
            m.set_build_option("dense_min_density", 0.4)
        oix, _ = helpers.taat_oracle((dp, dt, dw), n_terms)
        with m.SparseIndex(path, device=0) as ix:
            for k in {1, int(rng.integers(2, 200)), 1024}:
                for drop in (True, False):
                    try:
                        want = oix.search(qp, qt, qw, k, drop_df_eq_n=drop, threads=4)
                    except OverflowError:
                        with pytest.raises(Exception, match="OVERFLOW"):
                            ix.search_csr(qp, qt, qw, k, drop_df_eq_n=drop)
                        continue
                    helpers.assert_same_results(ix.search_csr(qp, qt, qw, k, drop_df_eq_n=drop), want, k)
            # the multi-GPU partitions of the same index, played on this one GPU: doc-range shards + the exact merge,
            # and term-range shard handles (each resident with its own term range only) + the reduction protocol
            k = int(rng.integers(1, 64))
            try:
                want = oix.search(qp, qt, qw, k, threads=4)
            except OverflowError:
                want = None
            if want is not None:
                G = int(rng.integers(1, min(ix.n_tiles, 4) + 1))
                lists = []
                for sh_i in range(G):
                    with m.SparseIndex(path, device=0, shard=sh_i, n_shards=G) as sh:
                        lists.append(sh.search_csr(qp, qt, qw, k))
                merged = ix.merge_lists(np.stack([l[0] for l in lists]), np.stack([l[2] for l in lists]),
                                        np.stack([l[3] for l in lists]), k)
                helpers.assert_same_results(merged, want, k)
                GT = int(rng.integers(1, 5))
                shards = [m.SparseIndex(path, device=0, term_shard=(g, GT)) for g in range(GT)]
                try:
                    helpers.assert_same_results(m.search_termshard_emulated_handles(shards, qp, qt, qw, k), want, k)
                finally:
                    for sh in shards:
                        sh.close()
        os.remove(path)


@pytest.mark.parametrize("dtype,vocab,k", [("float32", 32064, 128), ("float16", 128256, 128), ("float16", 3000, 256)])
def test_sparsifier_against_torch(m, dtype, vocab, k):
    """log(1 + relu) -> topk -> rint(x * 100) against plain PyTorch on the CPU (src/model.py:104, src/encode.py:69-75).
    Floating point: values within 1e-6 (f32) / equal after the fp16 rounding; integer weights equal except where
    v * 100 sits within float noise of a .5 boundary (f32 only); ids equal except inside exact value ties."""
    import torch

    from mllm_sparse_retrieval_amd.sparsify import sparsify_logits

    rng = np.random.default_rng(vocab)
    x = (rng.standard_normal((6, vocab)) * 4).astype(dtype)
    ids, vals, w = sparsify_logits(x, k)
    t = torch.from_numpy(x)
    ref = torch.log(1 + torch.relu(t))
    tv, ti = ref.topk(k, dim=-1)
    tv32 = tv.float().numpy()
    want_w = np.rint(tv32 * 100).astype(int)
    tol = 2e-6 if dtype == "float32" else 0.0
    assert np.abs(vals - tv32).max() <= tol + (1e-3 if dtype == "float16" else 0)  # torch's half log may differ by 1 ulp
    bad = w != want_w
    assert bad.mean() <= (0.002 if dtype == "float32" else 0.02)
    assert np.abs(w - want_w).max() <= 1
    # ids: same SET per row once exact ties at the k-th value are set aside
    for r in range(6):
        kth = tv32[r, -1]
        a = {int(i) for i, v in zip(ids[r], vals[r]) if v > kth + 1e-3}
        b = {int(i) for i, v in zip(ti[r].numpy(), tv32[r]) if v > kth + 1e-3}
        assert a == b
    assert (np.diff(vals, axis=1) <= 0).all()


def test_text_queries_tokenised_in_c(m, tmp_path):
    """msr_search_text (C tokenisation + counting + lookup) == Python tokenisation + msr_search_csr, on query strings
    built like src/search.py:419-422, including OOV tokens, odd whitespace and an empty string."""
    from mllm_sparse_retrieval_amd.searcher import tokenize_queries

    docs, (qp, qt, qw) = helpers.synth(4000, 32, 60, 25, 800, seed=19)
    terms = [f"ġt{i}" for i in range(800)]
    path = m.build_index_from_csr(str(tmp_path / "x.idx"), *docs, 800, term_strs=terms)
    queries = []
    for i in range(60):
        toks, vals = [terms[t] for t in qt[qp[i]:qp[i + 1]]], qw[qp[i]:qp[i + 1]] % 7
        q = ""
        for tok, v in zip(toks, vals):
            q += (" " + tok) * int(v)
        queries.append(q.strip())
    queries += ["", "   ", "unicorn  ġt5\\tġt5\\n ġt7 unicorn", "ġt1"]
    with m.SparseIndex(path, device=0) as ix:
        got = ix.search_text(queries, 10)
        p, toks, ws = tokenize_queries(queries)
        want = ix.search_csr(p, ix.lookup(toks), ws, 10)
        for a, b in zip(got, want):
            assert (a == b).all()
        assert got[3][60] == 0 and got[3][61] == 0 and got[3][62] > 0


def test_large_vocabulary_llama3_shape(m, tmp_path):
    # V = 128 256 (llama-3 llava-next vocabulary): seg_ptr rows of 0.5 MB per tile
    _case(m, tmp_path, 12000, 128, 300, 128, 128256, seed=128, tile_docs=0, ks=[10])
