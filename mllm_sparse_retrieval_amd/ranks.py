"""Retrieval metrics from exact ranks (SparseIndex.rank_docs): Recall@k for any k, MRR, MedR and MeanR, the numbers
image-text retrieval tables print beside R@1/5/10. A depth-limited run cannot give them exactly: a judged doc below the
search depth is missing from it. Recall follows the reference's rule (src/metrices.py:76-84, RecallMetrics._count): a
query is a hit at k when ANY of its targets is in the top k.
"""
from __future__ import annotations

import numpy as np

from .recall import RECALL_KS


def rank_metrics(ranks, t_ptr, n_docs, ks=RECALL_KS):
    """ranks: one exact rank per listed doc (0 = not ranked), t_ptr: query i owns ranks[t_ptr[i]:t_ptr[i + 1]].

    Per query `best` is the smallest positive rank among its targets. Returns
      recall[k]   share of the queries with 1 <= best <= k,
      mrr         mean of 1 / best (0 for a query without a positive rank),
      medr, meanr median / mean of best, a query without a positive rank entering as n_docs + 1,
      n_unranked  number of such queries,
      n_queries   queries with at least one target (the denominator of everything above)."""
    ranks = np.asarray(ranks, dtype=np.int64)
    t_ptr = np.asarray(t_ptr, dtype=np.int64)
    if t_ptr.ndim != 1 or len(t_ptr) < 1 or t_ptr[0] != 0 or t_ptr[-1] != len(ranks) or (np.diff(t_ptr) < 0).any():
        raise ValueError("malformed CSR target arrays")
    best = []
    for i in range(len(t_ptr) - 1):
        r = ranks[t_ptr[i]:t_ptr[i + 1]]
        if len(r) == 0:
            continue
        pos = r[r > 0]
        best.append(int(pos.min()) if len(pos) else 0)
    best = np.asarray(best, dtype=np.int64)
    n = len(best)
    if n == 0:
        return dict(recall={int(k): 0.0 for k in ks}, mrr=0.0, medr=0.0, meanr=0.0, n_unranked=0, n_queries=0)
    ranked = best > 0
    filled = np.where(ranked, best, int(n_docs) + 1)
    return dict(recall={int(k): float(np.count_nonzero(ranked & (best <= k))) / n for k in ks},
                mrr=float(np.sum(1.0 / best[ranked])) / n,
                medr=float(np.median(filled)), meanr=float(np.mean(filled)),
                n_unranked=int(np.count_nonzero(~ranked)), n_queries=n)
