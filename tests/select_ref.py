"""Exact numpy references for the selection and merge kernels (tests/test_select_merge.py, tests/test_launch_splits.py).

Everything here is integer arithmetic, float64, or numpy's correctly rounded float16 / float32 conversions: none of it
calls libmsr. tests/test_select_ref.py checks these helpers on the CPU against brute force."""
from __future__ import annotations

import numpy as np

NO_DOC = 0xFFFFFFFF


def merge_ref(ords, scores_u32, n, k):
    """Expected msr_merge_lists output for lists ords/scores [L, nq, k], counts n [L, nq].

    Entries j < clamp(n, 0, k) with a non-zero score take part (include/msr.h); the result is ranked by score
    descending, then ordinal ascending, padded with (0xFFFFFFFF, 0) past the hit count.
    -> (ords uint32 [nq, k], scores uint32 [nq, k], n int32 [nq])"""
    ords = np.asarray(ords, dtype=np.uint32)
    scores_u32 = np.asarray(scores_u32, dtype=np.uint32)
    n = np.asarray(n, dtype=np.int64)
    L, nq, _ = ords.shape
    o_out = np.full((nq, k), NO_DOC, dtype=np.uint32)
    s_out = np.zeros((nq, k), dtype=np.uint32)
    n_out = np.zeros(nq, dtype=np.int32)
    for q in range(nq):
        cand_o, cand_s = [], []
        for l in range(L):
            c = int(min(max(n[l, q], 0), k))
            s = scores_u32[l, q, :c].astype(np.int64)
            keep = s != 0
            cand_o.append(ords[l, q, :c].astype(np.int64)[keep])
            cand_s.append(s[keep])
        co, cs = np.concatenate(cand_o), np.concatenate(cand_s)
        order = np.lexsort((co, -cs))[:k]
        m = len(order)
        o_out[q, :m] = co[order]
        s_out[q, :m] = cs[order]
        n_out[q] = m
    return o_out, s_out, n_out


def dyadic(rng, shape, step=0.125, lim=2.0):
    """Multiples of `step` in [-lim, lim] as float32: with h * lim^2 / step^2 < 2^24 every product and partial sum of a
    row-by-row dot product is exact in f32 (and the values themselves are exact in fp16)."""
    m = int(round(lim / step))
    return (rng.integers(-m, m + 1, size=shape) * step).astype(np.float32)


def dense_topk_sparse_rows(q, rows, p_rows, n_docs, k):
    """Exact top-k of q @ P^T where P is zero except at the sorted row indices `rows` (holding `p_rows`).

    Scores are computed in float64 (exact for dyadic inputs); every other row scores exactly 0. Ranking: score
    descending, then row ascending, over all n_docs rows -> (idx uint32 [nq, k], f64 scores [nq, k])."""
    rows = np.asarray(rows, dtype=np.int64)
    assert (np.diff(rows) > 0).all()
    s = q.astype(np.float64) @ p_rows.astype(np.float64).T  # [nq, len(rows)]
    nq = q.shape[0]
    kk = min(k, n_docs)
    idx = np.zeros((nq, kk), dtype=np.int64)
    val = np.zeros((nq, kk), dtype=np.float64)
    listed = set(rows.tolist())
    for i in range(nq):
        pos = rows[s[i] > 0]
        pos_s = s[i][s[i] > 0]
        o = np.lexsort((pos, -pos_s))[:kk]
        top_o, top_s = list(pos[o]), list(pos_s[o])
        if len(top_o) < kk:
            # the zero run: the lowest rows that score exactly 0 (listed rows scoring 0 or unlisted rows)
            need = kk - len(top_o)
            zero_listed = set(rows[s[i] == 0].tolist())
            zs, r = [], 0
            while len(zs) < need and r < n_docs:
                if r in zero_listed or r not in listed:
                    zs.append(r)
                r += 1
            top_o += zs
            top_s += [0.0] * len(zs)
            if len(top_o) < kk:
                neg = rows[s[i] < 0]
                neg_s = s[i][s[i] < 0]
                o = np.lexsort((neg, -neg_s))[: kk - len(top_o)]
                top_o += list(neg[o])
                top_s += list(neg_s[o])
        idx[i] = top_o
        val[i] = top_s
    return idx.astype(np.uint32), val


def f32_keys(x):
    """The library's order-preserving f32 -> u32 map (include/msr.h)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def log1p_relu_f32(x):
    """float64 log of the f32 value 1 + relu(x) (the f32 sparsifier adds in f32, then takes logf) and one f32 ulp of
    the result, for f32 logits x."""
    y = np.float32(1) + np.maximum(np.asarray(x, dtype=np.float32), np.float32(0))  # numpy f32 add: correctly rounded
    v = np.log(y.astype(np.float64))
    v32 = v.astype(np.float32)
    ulp = (np.nextafter(v32, np.float32(np.inf)) - v32).astype(np.float64)
    return v, ulp


def log1p_relu_f16(x16):
    """f16(log(f16(1 + relu(x)))) for half logits, the half add and the final rounding correctly rounded, the log in
    float64 -> (expected half values, mask of inputs whose float64 log lies within one f32 ulp of a half rounding
    midpoint, where a faithfully rounded f32 logf may round the other way)."""
    x16 = np.asarray(x16, dtype=np.float16)
    y = np.float16(1) + np.maximum(x16, np.float16(0))  # numpy half add: correctly rounded
    v = np.log(y.astype(np.float64))
    want = v.astype(np.float16)
    # the half neighbour on the other side of v and the midpoint between them
    w64 = want.astype(np.float64)
    other = np.nextafter(want, np.where(w64 <= v, np.float16(np.inf), np.float16(-np.inf)).astype(np.float16))
    mid = (w64 + other.astype(np.float64)) / 2
    v32 = v.astype(np.float32)
    ulp = (np.nextafter(v32, np.float32(np.inf)) - v32).astype(np.float64)
    near = (np.abs(v - mid) <= ulp) & (v != 0)
    return want, near
