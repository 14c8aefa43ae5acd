"""numpy reference for msr_dense_rank_rows: exact ranks of listed rows by the definition in include/msr.h.

    keys[q, d]   the order-preserving u32 key of row d's score for query q (f32 handles: f32_chain.chain_scores +
                 f32_chain.f32_keys, the k-ordered fmaf chain)
    rank(q, t) = 0 if t == self[q],
                 else 1 + #{ d in [0, n), d != self[q] : keys[q, d] > keys[q, t] or (== and d < t) }

Every row is a hit: there is no "score 0 = not ranked" rule. Nothing here calls libmsr; every comparison against it is
exact equality.
"""
from __future__ import annotations

import numpy as np

from tests.f32_chain import chain_scores, f32_keys


def ranks_from_keys(keys, t_ptr, t_row, self_row=None):
    """keys uint32 [nq, n] -> (ranks uint32, keys uint32), indexed like t_row."""
    keys = np.asarray(keys, dtype=np.uint32)
    out_r = np.zeros(len(t_row), dtype=np.uint32)
    out_k = np.zeros(len(t_row), dtype=np.uint32)
    rows = np.arange(keys.shape[1])
    for q in range(len(t_ptr) - 1):
        k = keys[q]
        me = -1 if self_row is None else int(self_row[q])
        others = rows != me if me >= 0 else np.ones(len(rows), dtype=bool)
        for e in range(int(t_ptr[q]), int(t_ptr[q + 1])):
            t = int(t_row[e])
            out_k[e] = k[t]
            if t == me:
                continue
            out_r[e] = 1 + np.count_nonzero(others & ((k > k[t]) | ((k == k[t]) & (rows < t))))
    return out_r, out_k


def f32_ranks(q, p, t_ptr, t_row, self_row=None):
    """The reference for an f32 handle holding rows p, queries q."""
    return ranks_from_keys(f32_keys(chain_scores(q, p)), t_ptr, t_row, self_row)


def targets_csr(lists):
    """[[row, ...], ...] -> (t_ptr int64, t_row uint32)."""
    p = np.concatenate([[0], np.cumsum([len(r) for r in lists])]).astype(np.int64)
    return p, np.array([o for r in lists for o in r], dtype=np.uint32)


def random_targets(rng, nq, n, lo=0, hi=7):
    """lo..hi rows per query, drawn with replacement (duplicates occur)."""
    return [rng.integers(0, n, size=int(rng.integers(lo, hi + 1))).tolist() for _ in range(nq)]
