"""Shared test helpers: seeded workloads, an independent reader of the index file, oracle adapters."""
from __future__ import annotations

import struct

import numpy as np

SECTIONS = ["term_off", "term_str", "term_sorted", "df", "maxw", "doc_off", "doc_str", "seg_ptr", "postings",
            "dense_terms", "dense"]


def read_index_file(path):
    """Decode an MSRIDX01 file independently of libmsr.so (layout: csrc/msr_internal.h)."""
    raw = np.fromfile(path, dtype=np.uint8)
    b = raw.tobytes()
    magic = b[:8]
    assert magic == b"MSRIDX01", magic
    version, tile_docs = struct.unpack_from("<II", b, 8)
    n_docs, n_postings, n_vecs = struct.unpack_from("<QQQ", b, 16)
    n_terms, n_tiles, max_weight, n_dense = struct.unpack_from("<IIII", b, 40)
    ns = len(SECTIONS)
    off = struct.unpack_from(f"<{ns}Q", b, 56)
    size = struct.unpack_from(f"<{ns}Q", b, 56 + 8 * ns)
    (file_size,) = struct.unpack_from("<Q", b, 56 + 16 * ns)
    assert file_size == len(b)
    sec = {name: b[off[i] : off[i] + size[i]] for i, name in enumerate(SECTIONS)}
    term_off = np.frombuffer(sec["term_off"], dtype=np.uint64)
    doc_off = np.frombuffer(sec["doc_off"], dtype=np.uint64)
    terms = [sec["term_str"][int(term_off[i]) : int(term_off[i + 1]) - 1].decode("utf-8", "surrogateescape")
             for i in range(n_terms)]
    docs = [sec["doc_str"][int(doc_off[i]) : int(doc_off[i + 1]) - 1].decode("utf-8", "surrogateescape")
            for i in range(n_docs)]
    seg_ptr = np.frombuffer(sec["seg_ptr"], dtype=np.uint32).reshape(n_tiles, n_terms + 1)
    postings = np.frombuffer(sec["postings"], dtype=np.uint32)
    return dict(version=version, tile_docs=tile_docs, n_docs=n_docs, n_postings=n_postings, n_vecs=n_vecs,
                n_terms=n_terms, n_tiles=n_tiles, max_weight=max_weight, terms=terms, docs=docs, n_dense=n_dense,
                dense_terms=np.frombuffer(sec["dense_terms"], dtype=np.uint32),
                dense=np.frombuffer(sec["dense"], dtype=np.uint32).reshape(n_tiles, n_dense // 2, tile_docs),
                term_sorted=np.frombuffer(sec["term_sorted"], dtype=np.uint32),
                df=np.frombuffer(sec["df"], dtype=np.uint32), maxw=np.frombuffer(sec["maxw"], dtype=np.uint32),
                seg_ptr=seg_ptr, postings=postings)


def index_file_to_dense(ix):
    """Tile-major postings -> dense [n_docs, n_terms] int64 matrix (small indexes only)."""
    D = np.zeros((ix["n_docs"], ix["n_terms"]), dtype=np.int64)
    for tile in range(ix["n_tiles"]):
        for t in range(ix["n_terms"]):
            a, b = int(ix["seg_ptr"][tile, t]) * 4, int(ix["seg_ptr"][tile, t + 1]) * 4
            seg = ix["postings"][a:b]
            # a segment is a run of chunks (256 postings = 64 vecs); the order of postings INSIDE a chunk is free (the
            # builder arranges them by LDS bank, csrc/msr_index.cpp pass C), chunks follow each other in ordinal order
            real = []
            prev_max = -1
            for c0 in range(0, len(seg), 256):
                flat = seg[c0 : c0 + 256]
                nz = np.sort(flat[(flat >> 16) != 0] & 0xFFFF)  # weight 0 = padding
                assert len(flat) - len(nz) <= 3 or c0 + 256 >= len(seg), "only the last chunk is partial"
                assert len(nz) and nz[0] > prev_max, "chunks partition the segment in ordinal order"
                prev_max = int(nz[-1])
                real.append(flat[(flat >> 16) != 0])
            real = np.concatenate(real) if real else np.zeros(0, np.uint32)
            loc = (real & 0xFFFF).astype(np.int64)
            assert len(np.unique(loc)) == len(loc), "one posting per doc"
            D[tile * ix["tile_docs"] + loc, t] += (real >> 16).astype(np.int64)
    # dense head: slot s of pair s // 2 holds the weights of term dense_terms[s]; those terms have no segments
    for s, t in enumerate(ix["dense_terms"]):
        if t == 0xFFFFFFFF:
            assert not ((ix["dense"][:, s // 2, :] >> (16 * (s & 1))) & 0xFFFF).any()
            continue
        assert not D[:, t].any(), "a dense-head term must not have inverted lists"
        w = ((ix["dense"][:, s // 2, :] >> (16 * (s & 1))) & 0xFFFF).reshape(-1)[: ix["n_docs"]]
        D[:, t] = w.astype(np.int64)
    return D


def synth(n_docs, doc_nnz, n_queries, q_nnz, n_terms, seed):
    import mllm_sparse_retrieval_amd as m

    dp, dt, dw = m.synth_vectors(n_docs, doc_nnz, n_terms, seed=seed, threads=8)
    qp, qt, qw = m.synth_vectors(n_queries, q_nnz, n_terms, seed=seed + 1000003, threads=8)
    return (dp, dt, dw), (qp.astype(np.int64), qt.astype(np.int32), qw.astype(np.int32))


def taat_oracle(docs, n_terms, doc_ids=None):
    from oracle import taat

    dp, dt, dw = docs
    ix, order = taat.TaatIndex.from_rows_by_docid(dp, dt, dw, n_terms, doc_ids)
    return ix, order


def assert_same_results(got, want, k):
    """got = (ords u32, f32 scores, u32 scores, n) from libmsr; want = (ords i64 / -1 pad, scores i64, n)."""
    g_ord, g_f32, g_u32, g_n = got
    w_ord, w_sc, w_n = want
    assert (g_n == w_n).all(), np.flatnonzero(g_n != w_n)[:10]
    mask = np.arange(k)[None, :] < w_n[:, None]
    assert (g_ord.astype(np.int64)[mask] == w_ord[mask]).all(), "doc ordinals differ"
    assert (g_u32.astype(np.int64)[mask] == w_sc[mask]).all(), "exact scores differ"
    # f32 scores: (float)u32, round to nearest even (contract T5), bit for bit over the whole u32 range — numpy converts
    # int64 -> float32 by the same rule
    g_bits = np.ascontiguousarray(g_f32, dtype=np.float32).view(np.uint32)
    assert (g_bits[mask] == w_sc.astype(np.float32).view(np.uint32)[mask]).all(), "f32 scores differ"
    # padding: what merge_wave / merge_lists write for an empty slot (include/msr.h)
    assert (g_u32[~mask] == 0).all() and (g_f32[~mask] == 0.0).all() and (g_ord[~mask] == 0xFFFFFFFF).all()


def dense_oracle(q, p, k, tie_key=None):
    """numpy f32 inner products of the fp16-ROUNDED inputs (the storage precision of the reference's GPU faiss,
    src/search.py:257), ranked by (-score, row) — or by (-score, tie_key[row]) when a tie key is given (the fused
    hybrid kernel breaks exact dense ties by doc ordinal: DESIGN.md §5). Tolerance on scores: 1e-5 (f32 accumulation order)."""
    s = q.astype(np.float16).astype(np.float32) @ p.astype(np.float16).astype(np.float32).T
    tk = np.arange(s.shape[1]) if tie_key is None else np.asarray(tie_key, dtype=np.int64)
    order = np.lexsort((np.broadcast_to(tk, s.shape), -s), axis=1)[:, :k]
    return np.take_along_axis(s, order, axis=1), order


def oracle_hybrid(docs, n_terms, ids, qp, qt, qw, q, p, depth, alpha, sample, remove_query=False, qids=None,
                  dense_tie_key=None):
    """The reference's hybrid pipeline driven by the oracles for the queries in `sample`: C oracle sparse top-depth +
    numpy dense top-depth -> oracle.get_run_dict -> oracle.fuse (pinned to src/hybrid.py:32-53).
    -> ({qid: {doc: fused}}, qids of the sample)"""
    from oracle import oracle

    oix, order = taat_oracle(docs, n_terms, ids)
    sorted_ids = [ids[r] for r in order]
    sample = np.asarray(sample)
    sel = np.concatenate([np.arange(qp[i], qp[i + 1]) for i in sample]) if len(sample) else np.zeros(0, np.int64)
    sp = np.concatenate([[0], np.cumsum(qp[sample + 1] - qp[sample])]).astype(np.int64)
    wo, wsc, wn = oix.search(sp, qt[sel], qw[sel], depth, threads=16)
    sq = [str(int(i)) for i in sample] if qids is None else [qids[int(i)] for i in sample]
    o_sparse = oracle.get_run_dict(sq, [[float(np.float32(x)) for x in wsc[j, :wn[j]]] for j in range(len(sample))],
                                   [[sorted_ids[int(d)] for d in wo[j, :wn[j]]] for j in range(len(sample))], remove_query)
    dsc, didx = dense_oracle(q[sample], p, min(depth, p.shape[0]), dense_tie_key)
    o_dense = oracle.get_run_dict(sq, dsc, np.array([[ids[j] for j in row] for row in didx]), remove_query)
    return oracle.fuse([o_dense, o_sparse], [alpha, 1 - alpha]), sq


def assert_hybrid_matches(want, sq, sample, ords, fs, cnt, docid_of, k, tol=1e-5, tie=2e-6):
    worst = 0.0
    for j, i in enumerate(sample):
        ranked = sorted(want[sq[j]].items(), key=lambda kv: (-float(kv[1]), kv[0].encode()))[:k]
        assert cnt[i] == len(ranked), (sq[j], cnt[i], len(ranked))
        for r, (doc, score) in enumerate(ranked):
            worst = max(worst, abs(float(fs[i, r]) - float(score)))
            g = docid_of(int(ords[i, r]))
            if g != doc:  # only a near-tie in the fused score may swap neighbours
                assert g in want[sq[j]] and abs(float(want[sq[j]][g]) - float(score)) <= tie, (sq[j], r, g, doc)
    assert worst <= tol, worst


# ---- msr_hybrid_search_union against the reference's pipeline (tests/test_hybrid_union.py, tests/test_accum_edges.py)
UNION_TOL, UNION_TIE = 1e-5, 2e-6   # the fused-score tolerance and near-tie window of assert_hybrid_matches


def union_dense_lists(q, p, depth, prec, tie_key):
    """Dense top-depth (scores f32 [nq, depth'], rows) with ties to the lower tie_key, and the full score matrix."""
    from tests.f32_chain import chain_scores, f32_keys

    if prec == "f32":
        s = chain_scores(q, p)
    else:
        s = q.astype(np.float16).astype(np.float32) @ p.astype(np.float16).astype(np.float32).T
    keys = f32_keys(s).astype(np.int64)
    tk = np.broadcast_to(np.asarray(tie_key, np.int64), s.shape)
    order = np.lexsort((tk, -keys), axis=1)[:, :min(depth, p.shape[0])]
    return np.take_along_axis(s, order, axis=1), order, s


def union_oracle_runs(docs, n_terms, ids, qp, qt, qw, sample, depth, remove, qids, d_scores, d_rows):
    """The two run dicts of the reference's pipeline for the queries in `sample` (dense lists given, best first) and the
    exact integer sparse scores -> (o_sparse, o_dense, {qid: {doc: int}}, qids of the sample)."""
    from oracle import oracle

    oix, order = taat_oracle(docs, n_terms, ids)
    sorted_ids = [ids[r] for r in order]
    sample = np.asarray(sample)
    sel = np.concatenate([np.arange(qp[i], qp[i + 1]) for i in sample])
    sp = np.concatenate([[0], np.cumsum(qp[sample + 1] - qp[sample])]).astype(np.int64)
    wo, wsc, wn = oix.search(sp, qt[sel], qw[sel], depth, threads=16)
    sq = [qids[int(i)] for i in sample]
    s_docs = [[sorted_ids[int(d)] for d in wo[j, :wn[j]]] for j in range(len(sample))]
    o_sparse = oracle.get_run_dict(sq, [[float(np.float32(x)) for x in wsc[j, :wn[j]]] for j in range(len(sample))],
                                   s_docs, remove)
    o_dense = oracle.get_run_dict(sq, [list(map(float, r)) for r in d_scores],
                                  np.array([[ids[int(j)] for j in row] for row in d_rows]), remove)
    exact = {sq[j]: {d: int(x) for d, x in zip(s_docs[j], wsc[j, :wn[j]])} for j in range(len(sample))}
    return o_sparse, o_dense, exact, sq


def assert_union_arithmetic(res, alpha, smax_u=None):
    """One msr_hybrid_search_union result against tests/fusion_ref.refuse_union: every member's fused score, bit for bit,
    and the whole order (fused key descending, lower ordinal first) follow from out_src, out_sparse_u32, out_dense and
    out_range by the contract of include/msr.h. Exact equality, padding included."""
    from tests import fusion_ref

    ords, fs, cnt, src, su, de, rng = res[:7]
    want_ords, want_bits = fusion_ref.refuse_union(ords, cnt, src, su, de, rng, alpha, smax_u=smax_u)
    got_bits = np.ascontiguousarray(fs, dtype=np.float32).view(np.uint32)
    bad = np.flatnonzero((want_bits != got_bits).any(axis=1) | (want_ords != ords).any(axis=1))
    assert len(bad) == 0, ("fused bits or order differ from the contract in queries", bad[:10].tolist())


def check_union(res, sample, sq, o_sparse, o_dense, exact, alpha, depth, ix, dense_of):
    """Everything tests 1-3 of the union ask of one result: exact membership and fused order (assert_hybrid_matches at
    k = 2 x depth plus set equality), the side arrays, the padding, and union_to_runs against the oracle's run dicts —
    and, on EVERY query of the call, the fused score bits and the order recomputed from the call's own outputs by the
    contract's f32 operation sequence (assert_union_arithmetic).
    dense_of(j, doc) -> the f32 dense score the call must report for sample query j and that doc."""
    from mllm_sparse_retrieval_amd import fusion
    from oracle import oracle

    ords, fs, cnt, src, su, de, rng, _ = res
    assert_union_arithmetic(res, alpha)
    w = 2 * depth
    assert ords.shape == fs.shape == src.shape == su.shape == de.shape == (len(cnt), w) and rng.shape == (len(cnt), 4)
    want = oracle.fuse([o_dense, o_sparse], [alpha, 1 - alpha])
    assert_hybrid_matches(want, sq, sample, ords, fs, cnt, ix.docid, w, tol=UNION_TOL, tie=UNION_TIE)
    stat = fusion.fuse_statistic([o_dense, o_sparse], [alpha, 1 - alpha])
    bits_of = {"dense": 1, "sparse": 2, "fuse": 3}
    table = ix.docid_table()
    for j, i in enumerate(sample):
        c, qid = int(cnt[i]), sq[j]
        got_docs = table[ords[i, :c]].tolist()
        assert set(got_docs) == set(want[qid]) and len(set(got_docs)) == c, qid        # exact membership
        assert (np.diff(fs[i, :c]) <= 0).all()
        for r, doc in enumerate(got_docs):
            b = bits_of[stat[qid][doc].type]
            assert src[i, r] == b, (qid, doc, int(src[i, r]), b)
            assert su[i, r] == (exact[qid][doc] if b & 2 else 0), (qid, doc)
            if b & 1:
                assert np.float32(de[i, r]).view(np.uint32) == np.float32(dense_of(j, doc)).view(np.uint32), (qid, doc)
            else:
                assert de[i, r].view(np.uint32) == 0, (qid, doc)
        assert (ords[i, c:] == 0xFFFFFFFF).all() and (fs[i, c:].view(np.uint32) == 0).all()
        assert (src[i, c:] == 0).all() and (su[i, c:] == 0).all() and (de[i, c:].view(np.uint32) == 0).all()
        want_rng = [o_dense[qid]["max_score"], o_dense[qid]["min_score"], o_sparse[qid]["max_score"], o_sparse[qid]["min_score"]]
        assert (rng[i] == np.float32(want_rng)).all(), (qid, rng[i], want_rng)
    rows = np.asarray(sample)
    s_run, d_run, f_run = fusion.union_to_runs(sq, table, ords[rows], cnt[rows], fs[rows], src[rows], su[rows], de[rows],
                                               rng[rows])
    for got, ref, exact_bits in ((s_run, o_sparse, False), (d_run, o_dense, True)):
        for qid in sq:
            assert list(got[qid]["docs"]) == list(ref[qid]["docs"]), qid               # same docs, best first
            a = np.float32(list(got[qid]["docs"].values()))
            b = np.float32(list(ref[qid]["docs"].values()))
            assert (a.view(np.uint32) == b.view(np.uint32)).all() if exact_bits else (a == b).all(), qid
            assert np.float32(got[qid]["max_score"]) == np.float32(ref[qid]["max_score"]), qid
            assert np.float32(got[qid]["min_score"]) == np.float32(ref[qid]["min_score"]), qid
    assert all(set(f_run[qid]) == set(want[qid]) for qid in sq)
