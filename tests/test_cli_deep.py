"""search --deep end to end on the GPU: the sparse-only and the dense-only route write lists beyond 1024 whose first 1000
lines are the lines of the usual search, and hybrid --host_fusion --deep writes two deep lists and their whole fused
union (more than 1024 docs), equal to fusion.fuse of the two written lists."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_QUERIES = 300


@pytest.fixture(scope="module")
def m(built):
    import mllm_sparse_retrieval_amd as m

    return m


@pytest.fixture(scope="module")
def flickr_encode(m, tmp_path_factory):
    from mllm_sparse_retrieval_amd import cli

    root = tmp_path_factory.mktemp("cli_deep")
    enc, dense = str(root / "enc"), str(root / "dense")
    cli.main(["encode", "--synthetic", "flickr", "--n_images", "2000", "--sparse_output_dir", enc, "--threads", "4",
              "--dense_output_dir", dense, "--dense_dim", "64"])
    cli.main(["index", "--input", enc, "--threads", "4", "--impact", "--pretokenized"])
    with open(os.path.join(enc, "query.tsv")) as f, open(root / "queries.tsv", "w") as g:
        g.writelines(f.readlines()[:N_QUERIES])
    return root, enc, dense, str(root / "queries.tsv")


def _search(root, name, *args):
    from mllm_sparse_retrieval_amd import cli

    out_dir = str(root / name)
    cli.main(["search", "--query_type", "text", "--dataset_name", "flickr", "--quiet", "--save_dir", out_dir, *args])
    return out_dir


def _lines(path):
    """{qid: [line, ...]} of a run file, in file order."""
    by_q = {}
    with open(path) as f:
        for line in f:
            by_q.setdefault(line.split(" ", 1)[0], []).append(line)
    return by_q


def _hits(m, enc, queries):
    """Docs with a positive score per query of the file, from the index's own doc vectors: a doc is a hit when it holds
    one of the query's kept terms (in the vocabulary, not in every doc)."""
    from mllm_sparse_retrieval_amd.cli import _index_path, read_queries

    qids, texts = read_queries(queries)
    with m.SparseIndex(_index_path(enc), device=0) as ix:
        d_ptr, term, _ = ix.doc_vectors(np.arange(ix.n_docs, dtype=np.uint32))
        q_ptr, q_term, q_w = ix.encode_queries(texts)
        df = ix.df(np.arange(ix.n_terms, dtype=np.int32))
        n_docs = ix.n_docs
    doc_of = np.repeat(np.arange(n_docs), np.diff(d_ptr.astype(np.int64)))
    order = np.argsort(term, kind="stable")
    starts = np.searchsorted(term[order], np.arange(len(df) + 1))
    hits = {}
    for i, qid in enumerate(qids):
        mask = np.zeros(n_docs, dtype=bool)
        for e in range(int(q_ptr[i]), int(q_ptr[i + 1])):
            t = int(q_term[e])
            if t >= 0 and q_w[e] > 0 and df[t] < n_docs:
                mask[doc_of[order[starts[t]:starts[t + 1]]]] = True
        hits[qid] = int(mask.sum())
    return hits, n_docs


def test_sparse_only(m, flickr_encode):
    root, enc, _, queries = flickr_encode
    deep = _lines(os.path.join(_search(root, "s_deep", "--sparse_index", enc, "--queries", queries, "--deep", "--depth", "3000"),
                               "sparse.trec"))
    usual = _lines(os.path.join(_search(root, "s_1000", "--sparse_index", enc, "--queries", queries, "--depth", "1000"),
                                "sparse.trec"))
    hits, n_docs = _hits(m, enc, queries)
    assert len(hits) == N_QUERIES and set(deep) == set(usual) == {q for q, h in hits.items() if h > 0}
    assert max(hits.values()) > 1024                      # the test bites: lists the usual search cannot return
    for qid, rows in deep.items():
        assert len(rows) == min(3000, hits[qid]), qid
        assert rows[:1000] == usual[qid], qid


def test_dense_only(m, flickr_encode):
    root, _, dense, queries = flickr_encode
    for prec in ([], ["--use_gpu"]):
        tag = "fp16" if prec else "f32"
        deep = _lines(os.path.join(_search(root, "d_deep_" + tag, "--passage_reps", dense, "--queries", queries, "--deep",
                                           "--depth", "3000", *prec), "dense.trec"))
        usual = _lines(os.path.join(_search(root, "d_1000_" + tag, "--passage_reps", dense, "--queries", queries,
                                            "--depth", "1000", *prec), "dense.trec"))
        assert len(deep) == N_QUERIES and set(deep) == set(usual)
        for qid, rows in deep.items():
            assert len(rows) == 2000, qid                 # every row is a hit: min(3000, n)
            assert rows[:1000] == usual[qid], qid


def test_hybrid_host_fusion(m, flickr_encode):
    from mllm_sparse_retrieval_amd.fusion import fuse, read_trec_run

    root, enc, dense, queries = flickr_encode
    out = _search(root, "h_deep", "--sparse_index", enc, "--passage_reps", dense, "--queries", queries, "--host_fusion",
                  "--deep", "--depth", "1500", "--alpha", "0.5", "--batch_size", "100")
    sparse, dense_run, fused = (read_trec_run(os.path.join(out, n + ".trec")) for n in ("sparse", "dense", "fusion"))
    assert len(dense_run) == N_QUERIES and set(fused) == set(dense_run) and set(sparse) <= set(fused)
    assert all(len(v["docs"]) == 1500 for v in dense_run.values()) and max(len(v["docs"]) for v in sparse.values()) > 1024
    # the written lists in the types the search fused them in: dense scores are f32, sparse scores Python floats
    f32 = lambda r: {"docs": {d: np.float32(s) for d, s in r["docs"].items()}, "min_score": np.float32(r["min_score"]),  # noqa: E731
                     "max_score": np.float32(r["max_score"])}
    empty = {"docs": {}, "min_score": 0, "max_score": 0}
    want = fuse([{q: f32(r) for q, r in dense_run.items()}, {q: sparse.get(q, empty) for q in dense_run}], [0.5, 0.5])
    for qid, got in fused.items():
        assert got["docs"] == {d: float(s) for d, s in want[qid].items()}, qid   # (a run file holds float(score))
    assert max(len(v["docs"]) for v in fused.values()) > 1024
