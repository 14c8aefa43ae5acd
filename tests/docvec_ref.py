"""numpy reference for msr_doc_vectors: the doc-major CSR (ptr int64, term uint32, weight uint32) of listed docs.

    rows_of_matrix(D, ords)          rows of the doc matrix D (int64 [n_docs, n_terms], the corpus the index was built
                                     from): every nonzero entry of row ords[e], ascending term id, a repeated ordinal
                                     gets its own equal row
    rows_of_csr(dp, dt, dw, ords)    the same from the input CSR (rows sorted by term): the defining property of the call
    decode_index_file(f)             an independent streamed decoder of the index FILE (f = helpers.read_index_file): per
                                     tile the contiguous vec range [seg_ptr[tile][0], seg_ptr[tile][n_terms]), padding
                                     (weight 0) dropped, the term of vec v = upper bound of v in the tile's seg_ptr row
                                     minus one, the dense head merged in -> the CSR of every doc, by ordinal

Nothing here calls libmsr; every comparison against it is exact equality.
"""
from __future__ import annotations

import numpy as np

NO_TERM = 0xFFFFFFFF


def _csr(docs, terms, ws, n_docs):
    order = np.lexsort((terms, docs))
    ptr = np.concatenate([[0], np.cumsum(np.bincount(docs, minlength=n_docs))]).astype(np.int64)
    return ptr, terms[order].astype(np.uint32), ws[order].astype(np.uint32)


def take_rows(csr, ords):
    """Rows ords[e] of a CSR over all docs -> the CSR of the listed entries."""
    ptr, term, w = csr
    ords = np.asarray(ords, dtype=np.int64)
    lens = ptr[ords + 1] - ptr[ords]
    out_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    sel = np.concatenate([np.arange(ptr[o], ptr[o + 1]) for o in ords]) if len(ords) else np.zeros(0, np.int64)
    sel = sel.astype(np.int64)
    return out_ptr, term[sel], w[sel]


def matrix_csr(D):
    rows, cols = np.nonzero(D)
    return _csr(rows.astype(np.int64), cols.astype(np.int64), D[rows, cols].astype(np.int64), D.shape[0])


def rows_of_matrix(D, ords):
    ords = np.asarray(ords, dtype=np.int64)
    sub = D[ords] if len(ords) else np.zeros((0, D.shape[1]), np.int64)
    return matrix_csr(sub)


def rows_of_csr(dp, dt, dw, ords):
    return take_rows((np.asarray(dp, np.int64), np.asarray(dt, np.uint32), np.asarray(dw, np.uint32)), ords)


def decode_index_file(f):
    n_docs, n_terms, tile_docs = int(f["n_docs"]), int(f["n_terms"]), int(f["tile_docs"])
    vecs = f["postings"].reshape(-1, 4)
    docs, terms, ws = [], [], []
    for tile in range(int(f["n_tiles"])):
        row = f["seg_ptr"][tile].astype(np.int64)
        v = np.arange(row[0], row[n_terms])
        t = np.searchsorted(row, v, side="right") - 1          # steps over runs of empty segments that share one start
        p = vecs[row[0]:row[n_terms]].astype(np.int64)
        keep = (p >> 16) != 0                                  # padding first: its ordinals look real
        docs.append(tile * tile_docs + (p & 0xFFFF)[keep])
        terms.append(np.broadcast_to(t[:, None], p.shape)[keep])
        ws.append((p >> 16)[keep])
    for s, t in enumerate(f["dense_terms"]):
        if t == NO_TERM:
            continue
        w = ((f["dense"][:, s // 2, :].astype(np.int64) >> (16 * (s & 1))) & 0xFFFF).reshape(-1)[:n_docs]
        on = np.flatnonzero(w)
        docs.append(on)
        terms.append(np.full(len(on), int(t), np.int64))
        ws.append(w[on])
    docs, terms, ws = (np.concatenate(x).astype(np.int64) for x in (docs, terms, ws))
    assert docs.max(initial=-1) < n_docs
    return _csr(docs, terms, ws, n_docs)
