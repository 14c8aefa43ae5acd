"""numpy reference for msr_explain_docs, by the definition in include/msr.h.

    D = rank_ref.doc_matrix(docs CSR)       int64 [n_docs, n_terms], from the CSR the index was built from
    target entry e of query i owns len_i = q_ptr[i + 1] - q_ptr[i] slots from x_ptr[e]; slot j belongs to input entry
    q_ptr[i] + j (term tau, weight omega) and holds D[t, tau] when the entry counts (tau >= 0, omega > 0, not dropped
    as df == N with df taken from D), else 0.

Nothing here calls libmsr; every comparison against it is exact equality.
"""
from __future__ import annotations

import numpy as np


def x_ptr_of(qp, tp):
    qp, tp = np.asarray(qp, dtype=np.int64), np.asarray(tp, dtype=np.int64)
    return np.concatenate([[0], np.cumsum(np.repeat(np.diff(qp), np.diff(tp)))]).astype(np.int64)


def counts(qp, qt, qw, D, drop_df_eq_n=True):
    """bool per input entry: does it count?"""
    qt, qw = np.asarray(qt, dtype=np.int64), np.asarray(qw, dtype=np.int64)
    df = np.count_nonzero(D, axis=0)
    ok = (qt >= 0) & (qw > 0)
    if drop_df_eq_n:
        ok &= ~(df[np.where(qt >= 0, qt, 0)] == D.shape[0])
    return ok


def explain(qp, qt, qw, tp, to, D, drop_df_eq_n=True):
    """-> (x_ptr int64 [n_entries + 1], doc_w int64)."""
    qt = np.asarray(qt, dtype=np.int64)
    ok = counts(qp, qt, qw, D, drop_df_eq_n)
    xp = x_ptr_of(qp, tp)
    out = np.zeros(int(xp[-1]), dtype=np.int64)
    for i in range(len(qp) - 1):
        b, e = int(qp[i]), int(qp[i + 1])
        terms, keep = np.where(qt[b:e] >= 0, qt[b:e], 0), ok[b:e]
        for t in range(int(tp[i]), int(tp[i + 1])):
            out[xp[t]:xp[t + 1]] = np.where(keep, D[int(to[t]), terms], 0)
    return xp, out


def row_scores(qp, qw, tp, xp, doc_w):
    """sum_j max(omega_j, 0) * doc_w[x_ptr[e] + j] per target entry: the left side of the identity (Python ints)."""
    out = []
    for i in range(len(qp) - 1):
        w = [max(int(x), 0) for x in qw[int(qp[i]):int(qp[i + 1])]]
        for t in range(int(tp[i]), int(tp[i + 1])):
            out.append(sum(a * int(b) for a, b in zip(w, doc_w[int(xp[t]):int(xp[t + 1])])))
    return np.array(out, dtype=np.int64)
