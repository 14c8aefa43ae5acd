"""msr_hybrid_search_union (dense.hybrid_search_union, fusion.union_to_runs, search --fusion_union) on the GPU against
the reference's hybrid pipeline: C oracle sparse top-depth + dense top-depth -> oracle.get_run_dict -> oracle.fuse, the
pipeline of tests/test_hybrid_f32.py with its run dicts kept. The union call has to return EVERY doc of either depth
list (up to 2 x depth, which no other call can), in fused order, with each member's provenance and both of its scores.

Dense oracles. f32: the k-ordered fmaf chain (tests/f32_chain.py), ties to the lower ordinal. fp16, exact cases: passage
and query entries are multiples of 1/8 in [-2, 2] and h <= 256, so every product is a multiple of 1/64 and every partial
sum stays below 2^10: f32 accumulation is exact in any order and numpy's scores equal the MFMA's bit for bit."""
import os

import numpy as np
import pytest

from tests import helpers
from tests.f32_chain import f32_keys
from tests.helpers import check_union as _check_union
from tests.helpers import union_dense_lists as _dense_lists
from tests.helpers import union_oracle_runs as _oracle_runs

pytestmark = pytest.mark.gpu

TOL, TIE = helpers.UNION_TOL, helpers.UNION_TIE    # the project's fused-score tolerance and near-tie window
PAD = 0xFFFFFFFF


@pytest.fixture(scope="module")
def m(built):
    import mllm_sparse_retrieval_amd as m

    return m


# ------------------------------------------------------------------------------------------------------- oracles
def _rows(rng, n, h, prec, dup_every=0):
    if prec == "fp16":   # multiples of 1/8 in [-2, 2]: exact in fp16, products exact in f32 (module docstring)
        x = (rng.integers(-16, 17, (n, h)) / 8.0).astype(np.float32)
    else:
        x = rng.standard_normal((n, h)).astype(np.float32)
    if dup_every and n > dup_every:
        x[dup_every::dup_every] = x[0]  # bit-equal rows: exact dense ties that the depth boundary may cut
    return x


def _corpus(m, tmp_path, prec, n, tile, h, nq, seed, dup_every, n_terms=2000):
    docs, (qp, qt, qw) = helpers.synth(n, 48, nq, 30, n_terms, seed=seed)
    rng = np.random.default_rng(seed)
    ids = [str(int(x)) for x in rng.permutation(3 * n)[:n]]     # ids in no particular order: ordinals != rows
    path = m.build_index_from_csr(str(tmp_path / f"u{seed}{prec}.idx"), *docs, n_terms, doc_ids=ids, tile_docs=tile)
    p, q = _rows(rng, n, h, prec, dup_every), _rows(rng, nq, h, prec)
    return dict(docs=docs, qp=qp, qt=qt, qw=qw, ids=ids, path=path, p=p, q=q, n_terms=n_terms,
                qids=[ids[i] for i in range(nq)])                # query ids that ARE doc ids: remove_query acts


def _case(m, tmp_path, prec, n, tile, h, nq, depth, alpha, remove, seed, dup_every):
    from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_search_union, row_to_ordinal

    c = _corpus(m, tmp_path, prec, n, tile, h, nq, seed, dup_every)
    with m.SparseIndex(c["path"], device=0) as ix:
        dix = DenseIndex(c["p"], precision=prec)
        try:
            r2o = row_to_ordinal(ix, c["ids"])
            self_ord = r2o[:nq].astype(np.int32) if remove else None
            res = hybrid_search_union(ix, dix, c["qp"], c["qt"], c["qw"], c["q"], depth, alpha, r2o, self_ord)
            assert res[7]["fusion"] > 0 and res[7]["dense_select"] == 0, res[7]     # the candidate path
            d_sc, d_rows, s_all = _dense_lists(c["q"], c["p"], depth, prec, r2o)
            sample = np.arange(nq)
            o_sparse, o_dense, exact, sq = _oracle_runs(c["docs"], c["n_terms"], c["ids"], c["qp"], c["qt"], c["qw"], sample,
                                                        depth, remove, c["qids"], d_sc, d_rows)
            row_of = {d: r for r, d in enumerate(c["ids"])}
            _check_union(res, sample, sq, o_sparse, o_dense, exact, alpha, depth, ix, lambda j, doc: s_all[j, row_of[doc]])
            if prec == "f32":   # ... which are the bits of msr_dense_search_f32 on the same handle
                k_sc, k_rows = dix.search(c["q"], min(depth, n))
                assert (k_sc.view(np.uint32) == np.take_along_axis(s_all, k_rows, axis=1).view(np.uint32)).all()
            if remove:
                assert all(c["qids"][i] not in ix.docid_table()[res[0][i, :res[2][i]]].tolist() for i in range(nq))
        finally:
            dix.close()
    return res


# ------------------------------------------------------------------ 1-3: exact membership and side arrays, f32 and fp16
SHAPES = {"multi": (20000, 4096, 1000, 501), "single": (5000, 8192, 1000, 37)}


@pytest.mark.parametrize("prec", ["f32", "fp16"])
@pytest.mark.parametrize("shape", ["multi", "single"])
def test_union_exact(m, tmp_path, prec, shape):
    n, tile, depth, dup = SHAPES[shape]
    res = _case(m, tmp_path, prec, n, tile, 64, 40, depth, 0.5, True, seed=len(shape) + len(prec), dup_every=dup)
    assert res[2].max() > 1024        # more docs than any other call returns


@pytest.mark.parametrize("prec", ["f32", "fp16"])
@pytest.mark.parametrize("depth,h", [(400, 72), (1000, 64)])
def test_union_exact_second_round(m, tmp_path, monkeypatch, prec, depth, h):
    """depth 400: 5 tiles x 800 records stay in the registers of the fusion kernel; depth 1000: 5 x 2 000 = 10 000 records
    are more than its 512 x 16 register slots, so every pass and the member look-up read them from global memory."""
    monkeypatch.setenv("MSR_HYBRID_QUOTA", "3")   # every query's lists outgrow the quota: all go to the second round
    _case(m, tmp_path, prec, 20000, 4096, h, 40, depth, 0.5, True, seed=7, dup_every=301)


# ----------------------------------------------------------------------------------------------- 4: prefix property
@pytest.mark.parametrize("prec", ["f32", "fp16"])
@pytest.mark.parametrize("shape", ["multi", "single"])
def test_prefix_of_the_union_is_the_top_k(m, tmp_path, prec, shape):
    from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_search, hybrid_search_f32, hybrid_search_union, row_to_ordinal

    n, tile, depth, dup = SHAPES[shape]
    nq = 40
    c = _corpus(m, tmp_path, prec, n, tile, 64, nq, 17, dup)
    topk = hybrid_search_f32 if prec == "f32" else hybrid_search
    with m.SparseIndex(c["path"], device=0) as ix:
        dix = DenseIndex(c["p"], precision=prec)
        try:
            r2o = row_to_ordinal(ix, c["ids"])
            self_ord = r2o[:nq].astype(np.int32)
            ords, fs, cnt = hybrid_search_union(ix, dix, c["qp"], c["qt"], c["qw"], c["q"], depth, 0.5, r2o, self_ord,
                                                with_lists=False)[:3]
            for k in (65, 200, 1000):
                o, f, n_k, ms = topk(ix, dix, c["qp"], c["qt"], c["qw"], c["q"], depth, k, 0.5, r2o, self_ord)
                assert ms["fusion"] > 0 and ms["dense_select"] == 0      # the candidate-kernel path
                assert (n_k == np.minimum(cnt, k)).all()
                assert (o == ords[:, :k]).all(), k
                assert (f.view(np.uint32) == fs[:, :k].view(np.uint32)).all(), k
        finally:
            dix.close()


# --------------------------------------------------------------------------- 5, 6: the reference's shape at full size
@pytest.fixture(scope="module")
def ref_shape(m, tmp_path_factory):
    """The i->t run of scripts/search.sh: 25 010 caption docs x 5 000 image queries, H = 4096, depth 1000, remove_query."""
    from mllm_sparse_retrieval_amd import workloads
    from mllm_sparse_retrieval_amd.dense import row_to_ordinal

    n, nq = 25010, 5000
    docs, (qp, qt, qw), p, q = workloads.hybrid_vectors(n, nq, 4096)
    ids = [str(i) for i in range(n)]
    path = m.build_index_from_csr(str(tmp_path_factory.mktemp("i2t") / "x.idx"), *docs, 30000, doc_ids=ids)
    ix = m.SparseIndex(path, device=0)
    r2o = row_to_ordinal(ix, ids)
    c = dict(docs=docs, qp=qp, qt=qt, qw=qw, p=p, q=q, ids=ids, ix=ix, r2o=r2o, self_ord=r2o[:nq].astype(np.int32),
             qids=[str(i) for i in range(nq)], sample=np.sort(np.random.default_rng(3 + n).choice(nq, 64, replace=False)))
    yield c
    ix.close()


def test_reference_shape_f32(m, ref_shape):
    from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_search_union

    c = ref_shape
    depth, sample = 1000, c["sample"]
    dix = DenseIndex(c["p"], precision="f32")
    try:
        res = hybrid_search_union(c["ix"], dix, c["qp"], c["qt"], c["qw"], c["q"], depth, 0.5, c["r2o"], c["self_ord"])
        # dense lists of the sampled queries from msr_dense_search_f32 on the same handle (the fmaf chain, bit for bit;
        # an exact dense tie AT the depth boundary does not occur between random unit rows at H = 4096, so the row and
        # the ordinal rule keep the same docs)
        d_sc, d_rows = dix.search(c["q"][sample], depth)
        # ... except inside the list, where two bit-equal scores do turn up: the union lists them by ordinal, a flat index
        # by row. The same docs and scores, put in the declared order of the candidate path
        order = np.lexsort((c["r2o"][d_rows].astype(np.int64), -f32_keys(d_sc).astype(np.int64)), axis=1)
        d_sc, d_rows = np.take_along_axis(d_sc, order, axis=1), np.take_along_axis(d_rows, order, axis=1)
        o_sparse, o_dense, exact, sq = _oracle_runs(c["docs"], 30000, c["ids"], c["qp"], c["qt"], c["qw"], sample, depth,
                                                    True, c["qids"], d_sc, d_rows)
        score_of = [dict(zip(d_rows[j].tolist(), d_sc[j])) for j in range(len(sample))]
        _check_union(res, sample, sq, o_sparse, o_dense, exact, 0.5, depth, c["ix"], lambda j, doc: score_of[j][int(doc)])
        assert res[2].min() > 1024
        # 6: a sampled query searched alone returns the bits of the batched call
        qp, qt, qw = c["qp"], c["qt"], c["qw"]
        for i in sample[:6]:
            i = int(i)
            a, b = int(qp[i]), int(qp[i + 1])
            one = hybrid_search_union(c["ix"], dix, np.array([0, b - a]), qt[a:b], qw[a:b], c["q"][i:i + 1], depth, 0.5,
                                      c["r2o"], c["self_ord"][i:i + 1])
            for x, y in zip(one[:7], res[:7]):
                assert (x[0].view(np.uint32 if x.dtype == np.float32 else x.dtype) ==
                        y[i].view(np.uint32 if y.dtype == np.float32 else y.dtype)).all(), i
    finally:
        dix.close()


def test_reference_shape_fp16(m, ref_shape):
    """numpy and the MFMA accumulate in different orders, so a doc may sit on the other side of the dense depth boundary.
    Per query: every doc in the symmetric difference of the two unions has an oracle dense score within 2e-6 of the
    oracle's depth-th dense score, and the symmetric difference holds at most twice as many docs as there are OTHER oracle
    dense scores within 2e-6 of that boundary (the boundary's own doc not counted: none => equal unions). Docs in both:
    fused scores within 1e-5, order equal up to 2e-6 near-ties."""
    from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_search_union
    from oracle import oracle

    c = ref_shape
    depth, sample = 1000, c["sample"]
    dix = DenseIndex(c["p"])
    try:
        ords, fs, cnt, src, su, de, rng, ms = hybrid_search_union(c["ix"], dix, c["qp"], c["qt"], c["qw"], c["q"], depth, 0.5,
                                                                  c["r2o"], c["self_ord"])
    finally:
        dix.close()
    assert ms["fusion"] > 0 and ms["dense_select"] == 0
    d_sc, d_rows, s_all = _dense_lists(c["q"][sample], c["p"], depth, "fp16", c["r2o"])
    o_sparse, o_dense, exact, sq = _oracle_runs(c["docs"], 30000, c["ids"], c["qp"], c["qt"], c["qw"], sample, depth, True,
                                                c["qids"], d_sc, d_rows)
    want = oracle.fuse([o_dense, o_sparse], [0.5, 0.5])
    table = c["ix"].docid_table()
    worst = 0.0
    for j, i in enumerate(sample):
        qid, n_i = sq[j], int(cnt[i])
        got_docs = table[ords[i, :n_i]].tolist()
        got, ref = set(got_docs), set(want[qid])
        assert len(got) == n_i and qid not in got
        boundary = float(d_sc[j, -1])
        near = int((np.abs(s_all[j].astype(np.float64) - boundary) <= TIE).sum()) - 1   # (not the boundary's own doc)
        diff = got ^ ref
        assert all(abs(float(s_all[j, int(d)]) - boundary) <= TIE for d in diff), (qid, diff)
        assert len(diff) <= 2 * near, (qid, len(diff), near)
        ranked = [d for d, _ in sorted(want[qid].items(), key=lambda kv: (-float(kv[1]), kv[0].encode())) if d in got]
        common = [(r, d) for r, d in enumerate(got_docs) if d in ref]
        assert len(common) == len(ranked)
        for (r, g), doc in zip(common, ranked):
            worst = max(worst, abs(float(fs[i, r]) - float(want[qid][g])))
            assert g == doc or abs(float(want[qid][g]) - float(want[qid][doc])) <= TIE, (qid, r, g, doc)
        # provenance and sparse scores of the members both sides hold
        for r, g in common:
            if su[i, r]:
                assert src[i, r] & 2 and su[i, r] == exact[qid][g]
    assert worst <= TOL, worst


def test_steady_state(m, tmp_path):
    from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_search_union, row_to_ordinal

    c = _corpus(m, tmp_path, "f32", 9000, 4096, 100, 200, 31, 59)
    with m.SparseIndex(c["path"], device=0) as ix:
        dix = DenseIndex(c["p"], precision="f32")
        try:
            r2o = row_to_ordinal(ix, c["ids"])
            first = hybrid_search_union(ix, dix, c["qp"], c["qt"], c["qw"], c["q"], 300, 0.5, r2o)
            st = dix.stats()
            for _ in range(2):
                again = hybrid_search_union(ix, dix, c["qp"], c["qt"], c["qw"], c["q"], 300, 0.5, r2o)
                assert all((x.view(np.uint32 if x.dtype == np.float32 else x.dtype) ==
                            y.view(np.uint32 if y.dtype == np.float32 else y.dtype)).all() for x, y in zip(first[:7], again[:7]))
            assert dix.stats()["device_allocs"] == st["device_allocs"]
            lean = hybrid_search_union(ix, dix, c["qp"], c["qt"], c["qw"], c["q"], 300, 0.5, r2o, with_lists=False)
            assert lean[3] is None and lean[4] is None and lean[5] is None and lean[6] is None
            assert (lean[0] == first[0]).all() and (lean[1].view(np.uint32) == first[1].view(np.uint32)).all()
            assert dix.stats()["device_allocs"] == st["device_allocs"]
        finally:
            dix.close()


# ------------------------------------------------------------------------------------------------------ 7: misuse
def test_misuse_and_edges(m, tmp_path):
    import ctypes

    from mllm_sparse_retrieval_amd import _cabi
    from mllm_sparse_retrieval_amd._cabi import MsrError
    from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_search_union

    L = _cabi.lib()
    rng = np.random.default_rng(5)
    p, q = _rows(rng, 3, 40, "f32"), _rows(rng, 4, 40, "f32")
    dp = np.array([0, 1, 2, 3], dtype=np.uint64)
    dt, dw = np.array([0, 1, 0], np.uint32), np.array([3, 2, 1], np.uint32)
    path = m.build_index_from_csr(str(tmp_path / "i.idx"), dp, dt, dw, 2, tile_docs=4096)
    path12k = m.build_index_from_csr(str(tmp_path / "j.idx"), dp, dt, dw, 2, tile_docs=12288)
    qp, qt, qw = np.array([0, 1, 2, 3, 4]), np.array([0, 1, 0, 1]), np.array([1, 1, 1, 1])
    r2o = np.arange(3, dtype=np.uint32)
    d32, d16 = DenseIndex(p, precision="f32"), DenseIndex(p)
    try:
        with m.SparseIndex(path, device=0) as ix:
            cp, ct, cw = _cabi.as_csr(qp, qt, qw)
            ords, sc, n = np.zeros((4, 4), np.uint32), np.zeros((4, 4), np.float32), np.zeros(4, np.int32)
            ms = (ctypes.c_float * 4)()
            q16 = q.astype(np.float16).view(np.uint16)
            for dx, is_f32, qq, opener in ((d16, 1, q, b"msr_dense_open_f32"), (d32, 0, q16, b"msr_dense_open")):
                rc = L.msr_hybrid_search_union(ix._h, dx._h, _cabi.ptr(cp), _cabi.ptr(ct), _cabi.ptr(cw), _cabi.ptr(qq),
                                               is_f32, 4, 2, 0.5, 0, _cabi.ptr(r2o), None, _cabi.ptr(ords), _cabi.ptr(sc),
                                               _cabi.ptr(n), None, None, None, None, ms)
                assert rc == -1 and opener in L.msr_last_error(), L.msr_last_error()
            for depth in (0, 1025):
                with pytest.raises(MsrError) as e:
                    hybrid_search_union(ix, d32, qp, qt, qw, q, depth, 0.5, r2o)
                assert e.value.code == -8, depth  # MSR_E_RANGE
            with pytest.raises(MsrError) as e:
                hybrid_search_union(ix, d32, qp, qt, qw, q, 2, 0.5, np.array([0, 0, 2], np.uint32))
            assert e.value.code == -1 and "permutation" in str(e.value)
            o, f, c, s, u, d, r, _ = hybrid_search_union(ix, d32, np.zeros(1, np.int64), np.zeros(0, np.int32),
                                                         np.zeros(0, np.int32), np.zeros((0, 40), np.float32), 5, 0.5, r2o)
            assert o.shape == f.shape == s.shape == u.shape == d.shape == (0, 10) and c.shape == (0,) and r.shape == (0, 4)
            # depth beyond the 3-doc corpus: the union holds every doc; with a self doc, every other doc
            for dx in (d32, d16):
                o, f, c, s, u, d, r, _ = hybrid_search_union(ix, dx, qp, qt, qw, q, 10, 0.5, r2o)
                assert o.shape == (4, 20) and (c == 3).all() and all(sorted(o[i, :3].tolist()) == [0, 1, 2] for i in range(4))
                assert (s[:, :3] & 1).all() and (o[:, 3:] == PAD).all() and (s[:, 3:] == 0).all()
                o, f, c, s, u, d, r, _ = hybrid_search_union(ix, dx, qp, qt, qw, q, 10, 0.5, r2o,
                                                             self_ord=np.array([0, 1, 2, -1], np.int32))
                assert c.tolist() == [2, 2, 2, 3] and all(i not in o[i, :2].tolist() for i in range(3))
        with m.SparseIndex(path12k, device=0) as ix:     # a tile size without a candidate-kernel instance
            with pytest.raises(MsrError) as e:
                hybrid_search_union(ix, d32, qp, qt, qw, q, 2, 0.5, r2o)
            assert e.value.code == -1 and "tile" in str(e.value)
    finally:
        d32.close()
        d16.close()
    # a doc-range shard handle
    c = _corpus(m, tmp_path, "f32", 9000, 4096, 40, 4, 41, 0)
    dix = DenseIndex(c["p"], precision="f32")
    try:
        with m.SparseIndex(c["path"], device=0, shard=0, n_shards=2) as ix:
            with pytest.raises(MsrError) as e:
                hybrid_search_union(ix, dix, c["qp"], c["qt"], c["qw"], c["q"], 10, 0.5, np.arange(9000, dtype=np.uint32))
            assert e.value.code == -1 and "shard" in str(e.value)
    finally:
        dix.close()


# --------------------------------------------------------------------------------------------------------- 8: CLI
@pytest.fixture(scope="module")
def flickr_encode(m, tmp_path_factory):
    from mllm_sparse_retrieval_amd import cli

    root = tmp_path_factory.mktemp("cli")
    enc, dense = str(root / "enc"), str(root / "dense")
    cli.main(["encode", "--synthetic", "flickr", "--n_images", "2000", "--sparse_output_dir", enc, "--threads", "4",
              "--dense_output_dir", dense, "--dense_dim", "64"])
    cli.main(["index", "--input", enc, "--threads", "4", "--impact", "--pretokenized"])
    # the captions of the first 400 images as the query file: the host route's Python loop is the slow part of this test
    with open(os.path.join(enc, "query.tsv")) as f, open(root / "queries.tsv", "w") as g:
        g.writelines(f.readlines()[:2000])
    return root, enc, dense, str(root / "queries.tsv")


@pytest.mark.parametrize("prec", ["fp16", "f32"])
def test_cli_fusion_union_against_host_fusion(m, flickr_encode, capsys, prec):
    from mllm_sparse_retrieval_amd import cli
    from mllm_sparse_retrieval_amd.fusion import read_trec_run

    root, enc, dense, queries = flickr_encode
    capsys.readouterr()
    depth = 800
    for route, extra in (("union", ["--fusion_union", "--fusion_k", "7"]), ("host", ["--host_fusion"])):
        out_dir = str(root / f"{route}_{prec}")
        cli.main(["search", "--sparse_index", enc, "--passage_reps", dense, "--depth", str(depth), "--batch_size", "500",
                    "--alpha", "0.5", "--query_type", "text", "--dataset_name", "flickr", "--quiet", "--queries", queries,
                    "--qrels", os.path.join(enc, "qrels.csv"), "--save_dir", out_dir, *extra,
                    *(["--hybrid_f32"] if prec == "f32" else [])])
        out = capsys.readouterr().out
        for name in ("Dense reps recall", "Sparse reps recall", "Fusion/Hybrid reps recall"):
            assert any(line.startswith(name) for line in out.splitlines()), (route, name)
    run = {r: {name: read_trec_run(str(root / f"{r}_{prec}" / f"{name}.trec")) for name in ("sparse", "dense", "fusion")}
           for r in ("union", "host")}
    fa, fb = run["union"]["fusion"], run["host"]["fusion"]
    assert fa.keys() == fb.keys() and len(fb) == 2000
    assert max(len(v["docs"]) for v in fb.values()) > 1024      # the test bites: no other GPU route returns these
    sa, sb = run["union"]["sparse"], run["host"]["sparse"]
    assert sa.keys() == sb.keys()
    assert all(list(sa[q]["docs"]) == list(sb[q]["docs"]) for q in sa)
    assert all(np.array_equal(np.float32(list(sa[q]["docs"].values())), np.float32(list(sb[q]["docs"].values()))) for q in sa)
    da, db = run["union"]["dense"], run["host"]["dense"]
    assert da.keys() == db.keys()
    for q in fb:
        a, b = fa[q]["docs"], fb[q]["docs"]
        if prec == "f32":
            assert set(a) == set(b), q                            # the same doc set as the host route
            # dense.trec identical — up to the one declared difference: between BIT-EQUAL dense scores (common among
            # 2 000 f32 scores of 64-d rows) the candidate path lists the lower ordinal first, a flat index the lower row
            ua, ub = da[q]["docs"], db[q]["docs"]
            assert set(ua) == set(ub) and all(np.float32(ua[d]) == np.float32(ub[d]) for d in ua), q
            assert np.array_equal(np.float32(list(ua.values())), np.float32(list(ub.values()))), q
            assert all(x == y or np.float32(ub[x]) == np.float32(ub[y]) for x, y in zip(ua, ub)), q
        else:   # boundary docs under the rule of test_reference_shape_fp16, the host route's dense list as the oracle
            # (the dense scores this test can see are those of the docs either route lists: `near` = the OTHER ones of
            # them within 2e-6 of the host list's last score)
            dense_of = {**da[q]["docs"], **db[q]["docs"]}
            boundary = float(min(db[q]["docs"].values()))
            near = sum(abs(v - boundary) <= TIE for v in dense_of.values()) - 1
            for x, y, what in ((set(a), set(b), "fusion"), (set(da[q]["docs"]), set(db[q]["docs"]), "dense")):
                diff = x ^ y
                assert all(abs(dense_of[d] - boundary) <= TIE for d in diff if d in dense_of), (q, what)
                assert len(diff) <= 2 * near, (q, what, len(diff), near)
            dd_a, dd_b = da[q]["docs"], db[q]["docs"]              # the dense lists apart from boundary docs
            la, lb = [d for d in dd_a if d in dd_b], [d for d in dd_b if d in dd_a]
            assert all(x == y or abs(dd_b[x] - dd_b[y]) <= TIE for x, y in zip(la, lb)), q
            assert max(abs(dd_a[d] - dd_b[d]) for d in la) <= TOL, q
        common = [d for d in a if d in b]
        assert max(abs(a[d] - b[d]) for d in common) <= TOL, q
        ranked_b = [d for d in b if d in a]
        assert all(x == y or abs(b[x] - b[y]) <= TIE for x, y in zip(common, ranked_b)), q

