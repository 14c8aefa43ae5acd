"""search --doc_sets / --query_sets end to end on the GPU: five folds over a small synthetic corpus, the fold's queries
search the fold's docs only, on the sparse-only, the dense-only and the hybrid --host_fusion route. Every doc of a run
line is in its query's set; the sparse run equals the --deep run at depth n_docs filtered on the host and cut; the fused
run is fusion.fuse of the two written filtered lists; the refusals print their messages."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_QUERIES, N_FOLDS, DEPTH = 300, 5, 100


@pytest.fixture(scope="module")
def m(built):
    import mllm_sparse_retrieval_amd as m

    return m


@pytest.fixture(scope="module")
def corpus(m, tmp_path_factory):
    from mllm_sparse_retrieval_amd import cli
    from mllm_sparse_retrieval_amd.cli import _index_path, read_queries

    root = tmp_path_factory.mktemp("cli_filtered")
    enc, dense = str(root / "enc"), str(root / "dense")
    cli.main(["encode", "--synthetic", "flickr", "--n_images", "2000", "--sparse_output_dir", enc, "--threads", "4",
              "--dense_output_dir", dense, "--dense_dim", "64"])
    cli.main(["index", "--input", enc, "--threads", "4", "--impact", "--pretokenized"])
    with open(os.path.join(enc, "query.tsv")) as f, open(root / "queries.tsv", "w") as g:
        g.writelines(f.readlines()[:N_QUERIES])
    qids, _ = read_queries(str(root / "queries.tsv"))
    with m.SparseIndex(_index_path(enc), device=-1) as meta:
        docids = meta.docid_table().tolist()
    fold_of_doc = {d: "fold%d" % (j % N_FOLDS) for j, d in enumerate(docids)}
    fold_of_q = {q: "fold%d" % (i % N_FOLDS) for i, q in enumerate(qids) if i % 7 != 6}    # every 7th query: unfiltered
    with open(root / "doc_sets.tsv", "w") as f:
        f.writelines(f"{d}\t{s}\n" for d, s in fold_of_doc.items() if d != docids[3])      # one doc is in no set
    del fold_of_doc[docids[3]]
    with open(root / "query_sets.tsv", "w") as f:
        f.writelines(f"{q}\t{s}\n" for q, s in fold_of_q.items())
    return dict(root=root, enc=enc, dense=dense, queries=str(root / "queries.tsv"), qids=qids, docids=docids,
                fold_of_doc=fold_of_doc, fold_of_q=fold_of_q, sets=["--doc_sets", str(root / "doc_sets.tsv"), "--query_sets",
                                                                     str(root / "query_sets.tsv")])


def _search(root, name, *args):
    from mllm_sparse_retrieval_amd import cli

    out_dir = str(root / name)
    cli.main(["search", "--query_type", "text", "--dataset_name", "flickr", "--quiet", "--save_dir", out_dir, *args])
    return out_dir


def _run(path):
    from mllm_sparse_retrieval_amd.fusion import read_trec_run

    return read_trec_run(path)


def _lines(path):
    by_q = {}
    with open(path) as f:
        for line in f:
            by_q.setdefault(line.split(" ", 1)[0], []).append(line.split())
    return by_q


def _in_set(c, qid, doc):
    return qid not in c["fold_of_q"] or c["fold_of_doc"].get(doc) == c["fold_of_q"][qid]


def test_sparse_only(m, corpus):
    c = corpus
    n_docs = len(c["docids"])
    got = _lines(os.path.join(_search(c["root"], "s_f", "--sparse_index", c["enc"], "--queries", c["queries"], "--depth",
                                      str(DEPTH), *c["sets"]), "sparse.trec"))
    deep = _lines(os.path.join(_search(c["root"], "s_deep", "--sparse_index", c["enc"], "--queries", c["queries"], "--deep",
                                       "--depth", str(n_docs)), "sparse.trec"))
    assert got and set(got) <= set(deep)
    n_cut = 0
    for qid, rows in deep.items():
        want = [(r[2], r[4]) for r in rows if _in_set(c, qid, r[2])][:DEPTH]    # (docid, score) of the deep list, struck and cut
        have = [(r[2], r[4]) for r in got.get(qid, [])]
        assert have == want, qid
        assert all(_in_set(c, qid, d) for d, _ in have)
        n_cut += len([r for r in rows if _in_set(c, qid, r[2])]) > DEPTH
    assert n_cut > 0                                                            # lists that the depth really cuts
    assert not any(c["docids"][3] in [r[2] for r in rows] for q, rows in got.items() if q in c["fold_of_q"])   # in no set


def test_dense_only(m, corpus):
    c = corpus
    for prec in ([], ["--use_gpu"]):
        tag = "fp16" if prec else "f32"
        got = _lines(os.path.join(_search(c["root"], "d_f_" + tag, "--passage_reps", c["dense"], "--queries", c["queries"],
                                          "--depth", str(DEPTH), *prec, *c["sets"]), "dense.trec"))
        usual = _lines(os.path.join(_search(c["root"], "d_u_" + tag, "--passage_reps", c["dense"], "--queries", c["queries"],
                                            "--depth", "1000", *prec), "dense.trec"))
        assert len(got) == N_QUERIES
        for qid, rows in got.items():
            assert len(rows) == DEPTH and all(_in_set(c, qid, r[2]) for r in rows), qid   # a fold holds 400 rows > depth
            want = [(r[2], r[4]) for r in usual[qid] if _in_set(c, qid, r[2])][:DEPTH]
            if len(want) == DEPTH:                                              # the unfiltered top-1000 reaches that far
                assert [(r[2], r[4]) for r in rows] == want, qid
        assert any(q not in c["fold_of_q"] for q in got)


def test_hybrid_host_fusion(m, corpus):
    from mllm_sparse_retrieval_amd.fusion import fuse

    c = corpus
    out = _search(c["root"], "h_f", "--sparse_index", c["enc"], "--passage_reps", c["dense"], "--queries", c["queries"],
                  "--host_fusion", "--depth", str(DEPTH), "--alpha", "0.5", *c["sets"])
    sparse, dense_run, fused = (_run(os.path.join(out, n + ".trec")) for n in ("sparse", "dense", "fusion"))
    assert len(dense_run) == N_QUERIES and set(fused) == set(dense_run) and set(sparse) <= set(fused)
    for run in (sparse, dense_run, fused):
        for qid, v in run.items():
            assert all(_in_set(c, qid, d) for d in v["docs"]), qid
    # the sparse and the dense list are those of the single-route runs
    alone_s = _run(os.path.join(_search(c["root"], "h_s", "--sparse_index", c["enc"], "--queries", c["queries"], "--depth",
                                        str(DEPTH), *c["sets"]), "sparse.trec"))
    alone_d = _run(os.path.join(_search(c["root"], "h_d", "--passage_reps", c["dense"], "--queries", c["queries"], "--depth",
                                        str(DEPTH), "--use_gpu", *c["sets"]), "dense.trec"))
    assert sparse == alone_s and dense_run == alone_d
    f32 = lambda r: {"docs": {d: np.float32(s) for d, s in r["docs"].items()}, "min_score": np.float32(r["min_score"]),  # noqa: E731
                     "max_score": np.float32(r["max_score"])}
    empty = {"docs": {}, "min_score": 0, "max_score": 0}
    want = fuse([{q: f32(r) for q, r in dense_run.items()}, {q: sparse.get(q, empty) for q in dense_run}], [0.5, 0.5])
    for qid, got in fused.items():
        assert got["docs"] == {d: float(s) for d, s in want[qid].items()}, qid


def test_refusals_print_their_messages(m, corpus):
    from mllm_sparse_retrieval_amd import cli

    c = corpus
    base = ["search", "--query_type", "text", "--dataset_name", "flickr", "--quiet", "--queries", c["queries"]]
    for extra, words in (
            (["--sparse_index", c["enc"], "--passage_reps", c["dense"], *c["sets"]], ["filtered hybrid", "--host_fusion"]),
            (["--sparse_index", c["enc"], "--deep", "--depth", "2000", *c["sets"]], ["--deep", "--doc_sets"]),
            (["--sparse_index", c["enc"], "--explain", "3", *c["sets"]], ["--explain", "--doc_sets"]),
            (["--sparse_index", c["enc"], "--ranks", "--qrels", "x.csv", *c["sets"]], ["--ranks", "--doc_sets"]),
            (["--sparse_index", c["enc"], "--doc_sets", c["sets"][1]], ["--query_sets", "both"])):
        with pytest.raises(SystemExit) as e:
            cli.main(base + extra)
        assert isinstance(e.value.code, str) and all(w in e.value.code for w in words), e.value.code
    # a doc id the index does not know, a set the doc file does not define
    bad_docs = c["root"] / "bad_docs.tsv"
    bad_docs.write_text(open(c["sets"][1]).read() + "no-such-doc\tfold0\n")
    bad_q = c["root"] / "bad_q.tsv"
    bad_q.write_text(f"{c['qids'][0]}\tfold9\n")
    for route in (["--sparse_index", c["enc"]], ["--passage_reps", c["dense"]]):
        with pytest.raises(SystemExit) as e:
            cli.main(base + route + ["--doc_sets", str(bad_docs), "--query_sets", c["sets"][3]])
        assert isinstance(e.value.code, str) and "no-such-doc" in e.value.code
        with pytest.raises(SystemExit) as e:
            cli.main(base + route + ["--doc_sets", c["sets"][1], "--query_sets", str(bad_q)])
        assert isinstance(e.value.code, str) and "fold9" in e.value.code
