"""Vectorised numpy emulation of the f32 dense search's numeric contract (include/msr.h, msr_dense_search_f32):

    s = fmaf(q[h-1], p[h-1], ... fmaf(q[1], p[1], fmaf(q[0], p[0], +0.0f)))

fmaf(a, b, c) is the correctly rounded f32 of the exact a*b + c. In float64 the product of two f32 values is exact,
and TwoSum splits s64 + e = a*b + c exactly. Rounding s64 to f32 is then the correct result except in one case: s64
sits exactly on an f32 midpoint while e != 0, where the exact value lies on e's side of the midpoint and rounds there
instead of to even."""
from __future__ import annotations

import numpy as np


def fmaf(a, b, c):
    """Correctly rounded f32 a*b + c, elementwise with numpy broadcasting (finite inputs)."""
    a64 = np.asarray(a, dtype=np.float32).astype(np.float64)
    b64 = np.asarray(b, dtype=np.float32).astype(np.float64)
    c64 = np.asarray(c, dtype=np.float32).astype(np.float64)
    p = a64 * b64  # exact: 24 + 24 significant bits
    s = p + c64
    bb = s - p  # TwoSum: s + e == p + c exactly
    e = (p - (s - bb)) + (c64 - bb)
    r = s.astype(np.float32)
    r64 = r.astype(np.float64)
    # the f32 neighbour of r on s's side; s is a midpoint iff it lies exactly halfway between the two
    other = np.nextafter(r, np.where(r64 < s, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    mid = (r64 != s) & (r64 + other.astype(np.float64) == 2.0 * s)
    up = mid & (e > 0)
    down = mid & (e < 0)
    if up.any() or down.any():
        r = np.where(up, np.maximum(r, other), np.where(down, np.minimum(r, other), r))
    return r.astype(np.float32)


def chain_scores(q, p):
    """[nq, h] x [n, h] f32 -> [nq, n] f32 scores of the k-ordered fmaf chain from +0."""
    q = np.asarray(q, dtype=np.float32)
    p = np.asarray(p, dtype=np.float32)
    acc = np.zeros((q.shape[0], p.shape[0]), dtype=np.float32)
    for k in range(q.shape[1]):
        acc = fmaf(q[:, k, None], p[None, :, k], acc)
    return acc


def f32_keys(scores):
    """The library's order-preserving f32 -> u32 map (include/msr.h)."""
    u = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def topk(scores, k):
    """Top-k of every row by key, ties to the lower row -> (row indices uint32 [nq, k], keys uint32 [nq, k],
    hit counts int32 [nq]), padded like the C-ABI (0xFFFFFFFF / key 0) past min(k, n)."""
    keys = f32_keys(scores)
    nq, n = keys.shape
    kk = min(k, n)
    order = np.argsort(-keys.astype(np.int64), axis=1, kind="stable")[:, :kk]
    idx = np.full((nq, k), 0xFFFFFFFF, dtype=np.uint32)
    out = np.zeros((nq, k), dtype=np.uint32)
    idx[:, :kk] = order
    out[:, :kk] = np.take_along_axis(keys, order, axis=1)
    return idx, out, np.full(nq, kk, dtype=np.int32)
