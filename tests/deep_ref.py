"""numpy reference for the deep lists (msr_search_deep, msr_dense_search_deep; include/msr.h): the exact top-k of every
row of a u32 key matrix by (key descending, column ascending), padded like the C-ABI, and the planted corpora the GPU
tests use. Nothing here calls libmsr; every comparison against it is exact equality."""
from __future__ import annotations

import numpy as np

NO_COL = 0xFFFFFFFF


def topk_rows(keys, k, skip_zero=True):
    """keys [nq, n] (non-negative, < 2^32) -> (cols uint32 [nq, k], keys uint32 [nq, k], n_hit int32 [nq]): per row the k
    best columns by np.lexsort on (col, -key); with skip_zero the key-0 columns are not members (the sparse route's
    "score 0 is no hit"). Slots past n_hit hold 0xFFFFFFFF / 0."""
    keys = np.asarray(keys)
    nq, n = keys.shape
    idx = np.full((nq, k), NO_COL, dtype=np.uint32)
    out = np.zeros((nq, k), dtype=np.uint32)
    n_hit = np.zeros(nq, dtype=np.int32)
    cols = np.arange(n)
    for i in range(nq):
        row = keys[i].astype(np.int64)
        order = np.lexsort((cols, -row))
        if skip_zero:
            order = order[row[order] != 0]
        kk = min(k, len(order))
        idx[i, :kk] = order[:kk]
        out[i, :kk] = row[order[:kk]]
        n_hit[i] = kk
    return idx, out, n_hit


def tie_class(row, k):
    """Of one row of keys: (theta = the k-th best non-zero key, members with key == theta, how many of them the top-k
    takes); (0, 0, 0) when the row has at most k members (nothing is cut)."""
    row = np.asarray(row).astype(np.int64)
    live = np.sort(row[row != 0])[::-1]
    if len(live) <= k:
        return 0, 0, 0
    theta = int(live[k - 1])
    return theta, int((live == theta).sum()), int(k - (live > theta).sum())


# ---- planted corpora (doc-term matrices int64 [n_docs, n_terms], as tests/rank_ref.py builds them)
def two_weight_corpus(n_docs):
    """One term: weight 5 on every third ordinal, weight 3 elsewhere."""
    D = np.full((n_docs, 1), 3, dtype=np.int64)
    D[::3, 0] = 5
    return D


def flat_corpus(n_docs, weight=7):
    """One term with the same weight in every doc: every doc scores the same."""
    return np.full((n_docs, 1), weight, dtype=np.int64)


def bit31_corpus(n_docs, seed=0):
    """Term 0: stored weights 60 000 .. 65 535 in every doc but the last (df = N - 1, kept under the df == N filter);
    with a query weight of 40 000 every hit scores in [2^31, 2^32)."""
    rng = np.random.default_rng(seed)
    D = np.zeros((n_docs, 1), dtype=np.int64)
    D[:-1, 0] = rng.integers(60000, 65536, size=n_docs - 1)
    return D
