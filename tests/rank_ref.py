"""numpy reference for msr_rank_docs: exact scores and exact ranks of listed docs, by the definition in include/msr.h.

    D = doc_matrix(docs CSR)                int64 [n_docs, n_terms], from the CSR the index was built from
    Q = query_matrix(query CSR, D, drop)    int64 [nq, n_terms]: entries with term < 0 or weight <= 0 ignored, duplicate
                                            terms add, terms with df == N dropped when asked (df taken from D)
    S = Q @ D.T
    rank(q, t) = 0 if S[q, t] == 0 or t == self, else 1 + #{d != self : S[q, d] > S[q, t] or (== and d < t)}

Docs carry zero-padded ids ("%07d"), so ordinal == input row; open_index() asserts that through docid_table(). Nothing
here calls the search or the rank path of libmsr; every comparison against it is exact equality.
"""
from __future__ import annotations

import numpy as np


def doc_ids(n_docs):
    return ["%07d" % i for i in range(n_docs)]


def doc_matrix(dp, dt, dw, n_terms):
    dp = np.asarray(dp, dtype=np.int64)
    D = np.zeros((len(dp) - 1, n_terms), dtype=np.int64)
    rows = np.repeat(np.arange(len(dp) - 1), np.diff(dp))
    np.add.at(D, (rows, np.asarray(dt, dtype=np.int64)), np.asarray(dw, dtype=np.int64))
    return D


def query_matrix(qp, qt, qw, D, drop_df_eq_n=True):
    n_docs, n_terms = D.shape
    df = np.count_nonzero(D, axis=0)
    Q = np.zeros((len(qp) - 1, n_terms), dtype=np.int64)
    for i in range(len(qp) - 1):
        for e in range(int(qp[i]), int(qp[i + 1])):
            t, w = int(qt[e]), int(qw[e])
            if t < 0 or w <= 0:
                continue
            if drop_df_eq_n and df[t] == n_docs:
                continue
            Q[i, t] += w
    return Q


def scores(qp, qt, qw, D, drop_df_eq_n=True):
    return query_matrix(qp, qt, qw, D, drop_df_eq_n) @ D.T


def ranks(S, t_ptr, t_ord, self_ord=None):
    """-> (ranks int64, scores int64), indexed like t_ord."""
    n = len(t_ord)
    out_r, out_s = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    ords = np.arange(S.shape[1])
    for q in range(len(t_ptr) - 1):
        s = S[q]
        me = -1 if self_ord is None else int(self_ord[q])
        others = ords != me
        for e in range(int(t_ptr[q]), int(t_ptr[q + 1])):
            t = int(t_ord[e])
            out_s[e] = s[t]
            if s[t] == 0 or t == me:
                continue
            out_r[e] = 1 + np.count_nonzero(others & ((s > s[t]) | ((s == s[t]) & (ords < t))))
    return out_r, out_s


def csr(rows):
    """[[(a, b), ...], ...] -> (ptr int64, a int32, b int32)."""
    p = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return p, np.array([a for r in rows for a, _ in r], dtype=np.int32), np.array([b for r in rows for _, b in r], dtype=np.int32)


def targets_csr(lists):
    """[[ordinal, ...], ...] -> (t_ptr int64, t_ord uint32)."""
    p = np.concatenate([[0], np.cumsum([len(r) for r in lists])]).astype(np.int64)
    return p, np.array([o for r in lists for o in r], dtype=np.uint32)


def docs_to_csr(D):
    """int64 [n_docs, n_terms] -> doc-major CSR (ptr uint64, term uint32, weight uint32)."""
    rows, cols = np.nonzero(D)
    dp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=D.shape[0]))]).astype(np.uint64)
    return dp, cols.astype(np.uint32), D[rows, cols].astype(np.uint32)


def random_corpus(n_docs, n_terms, nnz, seed, head=4, head_p=0.6):
    """Term 0 in EVERY doc (the planted df == N term), terms 1..head in a share head_p of the docs (a dense head under
    the default build options), the rest of each row filled to `nnz` distinct terms; weights 1-255."""
    rng = np.random.default_rng(seed)
    D = np.zeros((n_docs, n_terms), dtype=np.int64)
    D[:, 0] = rng.integers(1, 256, size=n_docs)
    for t in range(1, head + 1):
        on = rng.random(n_docs) < head_p
        D[on, t] = rng.integers(1, 256, size=int(on.sum()))
    fill = np.argsort(rng.random((n_docs, n_terms - head - 1)), axis=1)[:, :nnz] + head + 1
    need = nnz - np.count_nonzero(D, axis=1)
    for i in range(n_docs):
        D[i, fill[i, :need[i]]] = rng.integers(1, 256, size=need[i])
    return D


def random_queries(nq, nnz, n_terms, seed, dirty=True):
    """`nnz` entries per query over distinct terms; with `dirty` one entry each is turned into an OOV term (-1), a zero
    weight, a negative weight and a repeat of the query's first term."""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(nq):
        terms = rng.choice(n_terms, size=nnz, replace=False)
        w = rng.integers(1, 51, size=nnz)
        row = [(int(t), int(x)) for t, x in zip(terms, w)]
        if dirty and nnz >= 8:
            row[1] = (-1, row[1][1])
            row[2] = (row[2][0], 0)
            row[3] = (row[3][0], -7)
            row[4] = (row[0][0], row[4][1])
        rows.append(row)
    return rows


def random_targets(nq, n_docs, seed, lo=0, hi=7):
    """lo..hi targets per query, drawn with replacement (duplicates occur) ..."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nq):
        n = int(rng.integers(lo, hi + 1))
        t = rng.integers(0, n_docs, size=n).tolist()
        if n >= 3:
            t[2] = t[0]  # ... and one planted
        out.append(t)
    return out


def open_index(m, path, D, tile_docs, device=0, dense_max_terms=None, **kw):
    """Build the index of D with zero-padded ids and open it; asserts ordinal == input row."""
    if dense_max_terms is not None:
        m.set_build_option("dense_max_terms", dense_max_terms)
    try:
        m.build_index_from_csr(str(path), *docs_to_csr(D), D.shape[1], doc_ids=doc_ids(D.shape[0]), tile_docs=tile_docs)
    finally:
        if dense_max_terms is not None:
            m.set_build_option("dense_max_terms", 16)
    ix = m.SparseIndex(str(path), device=device, **kw)
    assert ix.docid_table().tolist() == doc_ids(D.shape[0])
    return ix
