"""f32 hybrid search on the GPU (msr_hybrid_search_f32, dense.hybrid_search_f32, search --hybrid_f32) against the
reference's pipeline with an f32 dense side: oracle sparse top-depth + f32 dense top-depth (the k-ordered fmaf chain,
tests/f32_chain.py, or msr_dense_search_f32 on the same handle, which is pinned to that chain bit for bit) ->
oracle.get_run_dict -> oracle.fuse. Every back end (single-tile fused, multi-tile with and without a second round,
list-based), the reference's two shapes at H = 4096, batch invariance, near-duplicates below fp16 resolution, the handle
shared with msr_dense_search_f32, misuse, and the CLI on both hybrid routes."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers
from tests.f32_chain import chain_scores, f32_keys

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def m(built):
    import mllm_sparse_retrieval_amd as m

    return m


def _rows(rng, n, h, dup_every=0):
    x = rng.standard_normal((n, h)).astype(np.float32)
    if dup_every and n > dup_every:
        x[dup_every::dup_every] = x[0]  # bit-equal rows: exact dense ties that the depth boundary may cut
    return x


def _chain_lists(q, p, depth, tie_key=None):
    """f32 dense top-depth of the fmaf chain, ties to the lower tie_key (default: row) -> (scores, rows)."""
    s = chain_scores(q, p)
    keys = f32_keys(s).astype(np.int64)
    tk = np.broadcast_to(np.arange(p.shape[0]) if tie_key is None else np.asarray(tie_key, np.int64), s.shape)
    order = np.lexsort((tk, -keys), axis=1)[:, :min(depth, p.shape[0])]
    return np.take_along_axis(s, order, axis=1), order


def _pipeline(docs, n_terms, ids, qp, qt, qw, sample, depth, alpha, remove, qids, d_scores, d_rows):
    """The reference's hybrid pipeline for the queries in `sample`, with the given f32 dense lists ([len(sample)] rows
    best first): C oracle sparse top-depth -> oracle.get_run_dict (both runs) -> oracle.fuse. -> ({qid: {doc: fused}}, qids)"""
    from oracle import oracle

    oix, order = helpers.taat_oracle(docs, n_terms, ids)
    sorted_ids = [ids[r] for r in order]
    sample = np.asarray(sample)
    sel = np.concatenate([np.arange(qp[i], qp[i + 1]) for i in sample])
    sp = np.concatenate([[0], np.cumsum(qp[sample + 1] - qp[sample])]).astype(np.int64)
    wo, wsc, wn = oix.search(sp, qt[sel], qw[sel], depth, threads=16)
    sq = [qids[int(i)] for i in sample]
    o_sparse = oracle.get_run_dict(sq, [[float(np.float32(x)) for x in wsc[j, :wn[j]]] for j in range(len(sample))],
                                   [[sorted_ids[int(d)] for d in wo[j, :wn[j]]] for j in range(len(sample))], remove)
    o_dense = oracle.get_run_dict(sq, [list(map(float, r)) for r in d_scores],
                                  np.array([[ids[int(j)] for j in row] for row in d_rows]), remove)
    return oracle.fuse([o_dense, o_sparse], [alpha, 1 - alpha]), sq


def _backend(ms):
    if ms["dense_select"] > 0:
        return "list"
    return "multi" if ms["fusion"] > 0 else "fused"


def _case(m, tmp_path, n, tile, h, nq, depth, k, alpha, remove, seed, dup_every=0, expect="fused", n_terms=2000):
    """One corpus through hybrid_search_f32, every query against the pipeline with chain-based dense lists."""
    from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_search_f32, row_to_ordinal

    docs, (qp, qt, qw) = helpers.synth(n, 48, nq, 30, n_terms, seed=seed)
    rng = np.random.default_rng(seed)
    ids = [str(int(x)) for x in rng.permutation(3 * n)[:n]]     # ids in no particular order: ordinals != rows
    path = m.build_index_from_csr(str(tmp_path / f"h{seed}.idx"), *docs, n_terms, doc_ids=ids, tile_docs=tile)
    p, q = _rows(rng, n, h, dup_every), _rows(rng, nq, h)
    qids = [ids[i] for i in range(nq)]                            # query ids that ARE doc ids: remove_query acts
    with m.SparseIndex(path, device=0) as ix:
        dix = DenseIndex(p, precision="f32")
        try:
            r2o = row_to_ordinal(ix, ids)
            self_ord = r2o[:nq].astype(np.int32) if remove else None
            ords, fs, cnt, ms = hybrid_search_f32(ix, dix, qp, qt, qw, q, depth, k, alpha, r2o, self_ord)
            assert _backend(ms) == expect, ms
            # the tie rule of the DENSE depth list: lower ordinal on the two fused paths, lower row on the list path
            d_sc, d_rows = _chain_lists(q, p, depth, None if expect == "list" else r2o)
            sample = np.arange(nq)
            want, sq = _pipeline(docs, n_terms, ids, qp, qt, qw, sample, depth, alpha, remove, qids, d_sc, d_rows)
            helpers.assert_hybrid_matches(want, sq, sample, ords, fs, cnt, ix.docid, k)
            if remove:
                assert all(qids[i] not in [ix.docid(int(o)) for o in ords[i, :cnt[i]]] for i in range(nq))
        finally:
            dix.close()
    return ords, fs, cnt


# ------------------------------------------------------------------------------------------- single-tile fused path
@pytest.mark.parametrize("n,tile,h,k,depth,alpha,remove", [
    (700, 4096, 1, 1, 10, 0.5, False), (700, 8192, 40, 10, 1000, 0.3, True), (5000, 8192, 100, 64, 1000, 0.5, True),
    (5000, 8192, 256, 10, 10, 0.3, False), (8192, 8192, 40, 64, 10, 0.5, True), (4096, 4096, 100, 10, 1000, 0.3, False)])
def test_fused_single_tile(m, tmp_path, n, tile, h, k, depth, alpha, remove):
    _case(m, tmp_path, n, tile, h, 48, depth, k, alpha, remove, seed=n + h + k, dup_every=37, expect="fused")


# ------------------------------------------------------------------------------------------------ multi-tile path
@pytest.mark.parametrize("k", [65, 1000])
def test_multitile(m, tmp_path, k):
    _case(m, tmp_path, 20000, 4096, 64, 40, 1000, k, 0.5, True, seed=k, dup_every=501, expect="multi")


def test_multitile_second_round(m, tmp_path, monkeypatch):
    monkeypatch.setenv("MSR_HYBRID_QUOTA", "3")   # every query's lists outgrow the quota: all go to the second round
    _case(m, tmp_path, 20000, 4096, 72, 40, 400, 10, 0.5, True, seed=7, dup_every=301, expect="multi")


# ------------------------------------------------------------------------------------------------ list-based path
def test_list_based(m, tmp_path):
    # a tile size without a fused kernel instance (the fused paths take 4096 / 8192) sends the call down the list path
    _case(m, tmp_path, 15000, 12288, 48, 40, 300, 20, 0.5, True, seed=11, dup_every=211, expect="list")


def test_list_based_forced_in_child(m, tmp_path):
    """MSR_NO_FUSED_HYBRID (read once per process) forces the list path for an index the multi-tile path would take."""
    from mllm_sparse_retrieval_amd.dense import row_to_ordinal

    n, nq, h, depth, k, alpha, n_terms = 9000, 30, 40, 200, 10, 0.5, 2000
    docs, (qp, qt, qw) = helpers.synth(n, 48, nq, 30, n_terms, seed=21)
    ids = [f"{i:05d}" for i in range(n)]
    path = m.build_index_from_csr(str(tmp_path / "c.idx"), *docs, n_terms, doc_ids=ids, tile_docs=4096)
    rng = np.random.default_rng(21)
    p, q = _rows(rng, n, h, 97), _rows(rng, nq, h)
    np.savez(tmp_path / "in.npz", p=p, q=q, qp=qp, qt=qt, qw=qw)
    code = f"""
import sys, numpy as np
sys.path.insert(0, {ROOT!r})
import mllm_sparse_retrieval_amd as m
from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_search_f32, row_to_ordinal
d = np.load({str(tmp_path / "in.npz")!r})
with m.SparseIndex({path!r}, device=0) as ix:
    dix = DenseIndex(d["p"], precision="f32")
    r2o = row_to_ordinal(ix, [f"{{i:05d}}" for i in range({n})])
    ords, fs, cnt, ms = hybrid_search_f32(ix, dix, d["qp"], d["qt"], d["qw"], d["q"], {depth}, {k}, {alpha}, r2o)
    assert ms["dense_select"] > 0, ms
    dix.close()
np.savez({str(tmp_path / "out.npz")!r}, ords=ords, fs=fs, cnt=cnt)
"""
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300,
                   env=dict(os.environ, MSR_NO_FUSED_HYBRID="1"))
    got = np.load(tmp_path / "out.npz")
    d_sc, d_rows = _chain_lists(q, p, depth)                          # list path: dense ties to the lower ROW
    sample = np.arange(nq)
    qids = [str(i) for i in range(nq)]
    want, sq = _pipeline(docs, n_terms, ids, qp, qt, qw, sample, depth, alpha, False, qids, d_sc, d_rows)
    with m.SparseIndex(path, device=-1) as ixh:
        assert (row_to_ordinal(ixh, ids) == np.arange(n)).all()
        helpers.assert_hybrid_matches(want, sq, sample, got["ords"], got["fs"], got["cnt"], ixh.docid, k)


# ------------------------------------------------------------------- the reference's shapes at full size, H = 4096
@pytest.fixture(scope="module")
def ref_shapes(m, tmp_path_factory):
    """The i->t run of scripts/search.sh (25 010 caption docs x 5 000 image queries, depth 1000, remove_query) and the
    reverse t->i shape (5 000 docs x 25 010 queries), unit rows in f32 (not rounded to fp16), searched whole."""
    from mllm_sparse_retrieval_amd import workloads
    from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_search_f32, row_to_ordinal

    out = {}
    for name, n, nq, k, remove in (("i2t", 25010, 5000, 1000, True), ("t2i", 5000, 25010, 10, False)):
        docs, (qp, qt, qw), p, q = workloads.hybrid_vectors(n, nq, 4096)
        ids = [str(i) for i in range(n)]
        path = m.build_index_from_csr(str(tmp_path_factory.mktemp(name) / "x.idx"), *docs, 30000, doc_ids=ids)
        ix = m.SparseIndex(path, device=0)
        dix = DenseIndex(p, precision="f32")
        r2o = row_to_ordinal(ix, ids)
        self_ord = r2o[:nq].astype(np.int32) if remove else None
        res = hybrid_search_f32(ix, dix, qp, qt, qw, q, 1000, k, 0.5, r2o, self_ord)
        out[name] = dict(docs=docs, qp=qp, qt=qt, qw=qw, q=q, ids=ids, ix=ix, dix=dix, r2o=r2o, self_ord=self_ord, k=k,
                         remove=remove, res=res, sample=np.random.default_rng(len(name) + n).choice(nq, 64, replace=False))
    yield out
    for v in out.values():
        v["dix"].close()
        v["ix"].close()


@pytest.mark.parametrize("name,backend", [("i2t", "multi"), ("t2i", "fused")])
def test_reference_shapes_full(m, ref_shapes, name, backend):
    c = ref_shapes[name]
    ords, fs, cnt, ms = c["res"]
    assert _backend(ms) == backend, ms
    sample = np.sort(c["sample"])
    # f32 dense top-depth of the sampled queries from msr_dense_search_f32 on the same handle (the fmaf chain, bit for
    # bit; exact dense ties do not occur between random unit rows at H = 4096, so row and ordinal rule agree)
    d_sc, d_rows = c["dix"].search(c["q"][sample], 1000)
    qids = [str(i) for i in range(len(c["qp"]) - 1)]
    want, sq = _pipeline(c["docs"], 30000, c["ids"], c["qp"], c["qt"], c["qw"], sample, 1000, 0.5, c["remove"], qids,
                         d_sc, d_rows)
    helpers.assert_hybrid_matches(want, sq, sample, ords, fs, cnt, c["ix"].docid, c["k"])
    if c["remove"]:
        assert all(qids[i] not in [c["ix"].docid(int(o)) for o in ords[i, :cnt[i]]] for i in sample)


@pytest.mark.parametrize("name", ["i2t", "t2i"])
def test_batch_invariance(m, ref_shapes, name):
    """Each sampled query searched alone gives the bits of the full batch."""
    from mllm_sparse_retrieval_amd.dense import hybrid_search_f32

    c = ref_shapes[name]
    ords, fs, cnt, _ = c["res"]
    qp, qt, qw = c["qp"], c["qt"], c["qw"]
    for i in c["sample"][:12]:
        i = int(i)
        a, b = int(qp[i]), int(qp[i + 1])
        so = None if c["self_ord"] is None else c["self_ord"][i:i + 1]
        o1, f1, n1, _ = hybrid_search_f32(c["ix"], c["dix"], np.array([0, b - a]), qt[a:b], qw[a:b], c["q"][i:i + 1], 1000,
                                          c["k"], 0.5, c["r2o"], so)
        assert n1[0] == cnt[i] and (o1[0] == ords[i]).all() and (f1[0].view(np.uint32) == fs[i].view(np.uint32)).all(), i


# ------------------------------------------------------------------------------------- not fp16 relabelled
def test_near_duplicates_below_fp16_resolution(m, tmp_path):
    """Eight passages one fp16 row apart by less than its resolution straddle the dense depth boundary (depth 4): f32
    ranks them by their true scores and keeps the four highest (the highest ordinals), fp16 sees one eight-way tie and
    keeps the four lowest ordinals. The f32 route matches the f32 pipeline; the fp16 route does not."""
    from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_search, hybrid_search_f32, row_to_ordinal

    n, h, depth, k, nq, n_terms = 700, 256, 4, 64, 1, 500
    rng = np.random.default_rng(13)
    b = (rng.uniform(2.0 ** -6, 1.0, h) * rng.choice([-1.0, 1.0], h)).astype(np.float16).astype(np.float32)
    p = (0.05 * rng.standard_normal((n, h))).astype(np.float32)        # every other passage scores far below
    p[:8] = b[None, :] * (1 + np.arange(8)[:, None] * 2.0 ** -16)       # rows 0..7: one fp16 row, eight f32 rows
    assert (p[:8].astype(np.float16) == b.astype(np.float16)).all()
    q = (b / np.linalg.norm(b))[None, :].astype(np.float32)
    # sparse side: rows 0..7 hold terms 0-99 only, every other row and the query terms 100-499, so that the near-duplicates
    # enter the union through the dense list alone
    nnz = 12
    dp = np.arange(0, n * nnz + 1, nnz, dtype=np.uint64)
    dt = np.concatenate([rng.choice(100, nnz, replace=False) if i < 8 else 100 + rng.choice(400, nnz, replace=False)
                         for i in range(n)]).astype(np.uint32)
    dw = rng.integers(1, 300, n * nnz).astype(np.uint32)
    docs = (dp, dt, dw)
    qp = np.array([0, 10], np.int64)
    qt = (100 + rng.choice(400, 10, replace=False)).astype(np.int32)
    qw = rng.integers(1, 50, 10).astype(np.int32)
    ids = [f"{i:04d}" for i in range(n)]                                # ordinal = row
    path = m.build_index_from_csr(str(tmp_path / "nd.idx"), *docs, n_terms, doc_ids=ids, tile_docs=4096)
    with m.SparseIndex(path, device=0) as ix:
        r2o = row_to_ordinal(ix, ids)
        d32, d16 = DenseIndex(p, precision="f32"), DenseIndex(p)
        try:
            o32, f32s, c32, ms = hybrid_search_f32(ix, d32, qp, qt, qw, q, depth, k, 0.5, r2o)
            o16, f16s, c16, _ = hybrid_search(ix, d16, qp, qt, qw, q, depth, k, 0.5, r2o)
        finally:
            d32.close()
            d16.close()
        assert _backend(ms) == "fused"
        d_sc, d_rows = _chain_lists(q, p, depth, r2o)
        assert sorted(d_rows[0].tolist()) == [4, 5, 6, 7]
        want, sq = _pipeline(docs, n_terms, ids, qp, qt, qw, np.arange(nq), depth, 0.5, False, ["q"], d_sc, d_rows)
        helpers.assert_hybrid_matches(want, sq, np.arange(nq), o32, f32s, c32, ix.docid, k)
        got32, got16 = set(o32[0, :c32[0]].tolist()), set(o16[0, :c16[0]].tolist())
        assert {4, 5, 6, 7} <= got32 and not ({0, 1, 2, 3} & got32)
        assert {0, 1, 2, 3} <= got16 and not ({4, 5, 6, 7} & got16)   # the fp16 route cut the other half of the tie
        with pytest.raises(AssertionError):
            helpers.assert_hybrid_matches(want, sq, np.arange(nq), o16, f16s, c16, ix.docid, k)


# ---------------------------------------------------------------------------------------- one handle, two calls
def test_one_handle_dense_and_hybrid(m, tmp_path):
    from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_search_f32, row_to_ordinal

    n, nq, h, n_terms = 9000, 200, 100, 2000
    docs, (qp, qt, qw) = helpers.synth(n, 48, nq, 30, n_terms, seed=31)
    rng = np.random.default_rng(31)
    p, q = _rows(rng, n, h, 59), _rows(rng, nq, h)
    path = m.build_index_from_csr(str(tmp_path / "o.idx"), *docs, n_terms, tile_docs=4096)
    with m.SparseIndex(path, device=0) as ix:
        dix = DenseIndex(p, precision="f32")
        try:
            before = dix.search_keys(q, 50)
            r2o = row_to_ordinal(ix, [str(i) for i in range(n)])
            first = hybrid_search_f32(ix, dix, qp, qt, qw, q, 300, 20, 0.5, r2o)
            st = dix.stats()
            for _ in range(2):
                again = hybrid_search_f32(ix, dix, qp, qt, qw, q, 300, 20, 0.5, r2o)
                assert all((x == y).all() for x, y in zip(first[:3], again[:3]))
            assert dix.stats()["device_allocs"] == st["device_allocs"]
            after = dix.search_keys(q, 50)
            assert all((x == y).all() for x, y in zip(before, after))
        finally:
            dix.close()


# ------------------------------------------------------------------------------------------------------ misuse
def test_misuse_and_edges(m, tmp_path):
    from mllm_sparse_retrieval_amd import _cabi
    from mllm_sparse_retrieval_amd._cabi import MsrError
    from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_search_f32

    L = _cabi.lib()
    rng = np.random.default_rng(5)
    p, q = _rows(rng, 3, 40), _rows(rng, 4, 40)
    dp = np.array([0, 1, 2, 3], dtype=np.uint64)
    path = m.build_index_from_csr(str(tmp_path / "i.idx"), dp, np.array([0, 1, 0], np.uint32),
                                  np.array([3, 2, 1], np.uint32), 2, tile_docs=4096)
    qp, qt, qw = np.array([0, 1, 2, 3, 4]), np.array([0, 1, 0, 1]), np.array([1, 1, 1, 1])
    r2o = np.arange(3, dtype=np.uint32)
    d32, d16, d32x = DenseIndex(p, precision="f32"), DenseIndex(p), DenseIndex(_rows(rng, 4, 40), precision="f32")
    try:
        with m.SparseIndex(path, device=0) as ix:
            # an fp16 handle: refused in Python and in the C-ABI, with a message that points to msr_hybrid_search
            with pytest.raises(ValueError):
                hybrid_search_f32(ix, d16, qp, qt, qw, q, 2, 2, 0.5, r2o)
            cp, ct, cw = _cabi.as_csr(qp, qt, qw)
            ords, sc, n = np.zeros((4, 2), np.uint32), np.zeros((4, 2), np.float32), np.zeros(4, np.int32)
            ms = (ctypes.c_float * 4)()
            rc = L.msr_hybrid_search_f32(ix._h, d16._h, _cabi.ptr(cp), _cabi.ptr(ct), _cabi.ptr(cw), _cabi.ptr(q), 4, 2, 2,
                                         0.5, 0, _cabi.ptr(r2o), None, _cabi.ptr(ords), _cabi.ptr(sc), _cabi.ptr(n), ms)
            assert rc == -1 and b"msr_hybrid_search" in L.msr_last_error()
            for depth, k in ((0, 2), (1025, 2), (2, 0), (2, 1025)):
                with pytest.raises(MsrError) as e:
                    hybrid_search_f32(ix, d32, qp, qt, qw, q, depth, k, 0.5, r2o)
                assert e.value.code == -8, (depth, k)  # MSR_E_RANGE
            with pytest.raises(MsrError) as e:
                hybrid_search_f32(ix, d32, qp, qt, qw, q, 2, 2, 0.5, np.array([0, 0, 2], np.uint32))
            assert e.value.code == -1 and "permutation" in str(e.value)
            with pytest.raises(MsrError) as e:  # 4 dense rows against 3 sparse docs
                hybrid_search_f32(ix, d32x, qp, qt, qw, q, 2, 2, 0.5, np.arange(4, dtype=np.uint32))
            assert e.value.code == -1
            with pytest.raises(ValueError):
                hybrid_search_f32(ix, d32, qp, qt, qw, np.zeros((4, 41), np.float32), 2, 2, 0.5, r2o)
            o, f, c, _ = hybrid_search_f32(ix, d32, np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32),
                                           np.zeros((0, 40), np.float32), 5, 3, 0.5, r2o)
            assert o.shape == (0, 3) and f.shape == (0, 3) and c.shape == (0,)
            # depth and k beyond the 3-doc corpus: the union holds every doc, fused scores of the f32 lists
            o, f, c, _ = hybrid_search_f32(ix, d32, qp, qt, qw, q, 10, 10, 0.5, r2o)
            assert (c == 3).all() and all(sorted(o[i, :3].tolist()) == [0, 1, 2] for i in range(4))
    finally:
        d32.close()
        d16.close()
        d32x.close()


# --------------------------------------------------------------------------------------------------------- CLI
def test_cli_hybrid_f32_both_routes(m, tmp_path, capsys):
    from mllm_sparse_retrieval_amd import cli
    from mllm_sparse_retrieval_amd.fusion import read_trec_run

    enc, dense = str(tmp_path / "enc"), str(tmp_path / "dense")
    cli.main(["encode", "--synthetic", "flickr", "--n_images", "300", "--sparse_output_dir", enc, "--threads", "4",
              "--dense_output_dir", dense, "--dense_dim", "64"])
    cli.main(["index", "--input", enc, "--threads", "4", "--impact", "--pretokenized"])
    capsys.readouterr()
    outs = {}
    for route, extra in (("gpu", []), ("host", ["--host_fusion"])):
        cli.main(["search", "--sparse_index", enc, "--passage_reps", dense, "--depth", "100", "--batch_size", "500",
                  "--alpha", "0.5", "--query_type", "text", "--dataset_name", "flickr", "--hybrid_f32",
                  "--qrels", os.path.join(enc, "qrels.csv"), "--save_dir", str(tmp_path / route), *extra])
        outs[route] = capsys.readouterr().out
        for name in ("Dense reps recall", "Sparse reps recall", "Fusion/Hybrid reps recall"):
            assert any(line.startswith(name) for line in outs[route].splitlines()), (route, name)
    for name in ("sparse.trec", "dense.trec"):
        a, b = read_trec_run(str(tmp_path / "gpu" / name)), read_trec_run(str(tmp_path / "host" / name))
        assert a.keys() == b.keys()
        assert all(list(a[q]["docs"]) == list(b[q]["docs"]) for q in a), name
        assert all(np.array_equal(np.float32(list(a[q]["docs"].values())), np.float32(list(b[q]["docs"].values())))
                   for q in a), name
    fa, fb = read_trec_run(str(tmp_path / "gpu" / "fusion.trec")), read_trec_run(str(tmp_path / "host" / "fusion.trec"))
    for q in fb:   # the GPU run keeps the best --fusion_k of the union; scores within 1e-5, order equal up to near-ties
        da, db = fa[q]["docs"], fb[q]["docs"]
        assert set(da) <= set(db) and len(da) == min(len(db), 1000)
        assert max(abs(da[d] - db[d]) for d in da) <= 1e-5
        ra, rb = list(da)[:10], list(db)[:10]
        assert all(x == y or abs(db[x] - db[y]) <= 2e-6 for x, y in zip(ra, rb))
