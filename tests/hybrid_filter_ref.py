"""numpy reference for filtered deep hybrid search (msr_hybrid_deep_filtered, include/msr.h, identity (b)): a filtered
query's result is what an index holding only the docs of its set would give. Plain numpy on top of tests/fusion_ref.fuse;
nothing here calls libmsr, and every comparison against it is exact equality.

    fuse(S, D, member, q_set, depth, alpha, self_ord)   per query: restrict S and D to the columns of the query's set M (all
        columns when q_set[i] < 0), move self_ord to its position in M (or to -1 when it is no member), run
        fusion_ref.fuse on that sub-corpus, map every ordinal back. -> fusion_ref.Fused, laid out as fuse() lays it out.
    standard_sets(n, depth, seed)   the doc sets every test of the feature covers, as a bool [8, n] matrix (SET_NAMES).
"""
from __future__ import annotations

import numpy as np

from tests import fusion_ref as fr

SET_NAMES = ("full", "empty", "last doc", "third tile", "below depth", "below depth + 1", "half", "tenth")


def standard_sets(n, depth, seed=5):
    """full | empty | the single doc n - 1 | ordinals >= 8192 (with 4096-doc tiles: only the ragged third tile of 9 001 docs)
    | ordinals < depth | ordinals < depth + 1 | a random half | a random tenth."""
    rng = np.random.default_rng(seed)
    o = np.arange(n)
    m = np.stack([np.ones(n, bool), np.zeros(n, bool), o == n - 1, o >= 8192, o < depth, o < depth + 1, rng.random(n) < 0.5,
                  rng.random(n) < 0.1])
    m.setflags(write=False)
    return m


def fuse(S, D, member, q_set, depth, alpha, self_ord=None):
    """S int [nq, n], D f32 [nq, n] by ordinal; member bool [n_sets, n]; q_set int [nq] in [-1, n_sets). -> fr.Fused."""
    S = np.asarray(S, dtype=np.int64)
    D = np.asarray(D, dtype=np.float32)
    member = np.asarray(member, dtype=bool).reshape(-1, S.shape[1])
    nq, n = S.shape
    w = 2 * depth
    out = fr.Fused(np.full((nq, w), fr.PAD, np.uint32), np.zeros((nq, w), np.uint32), np.zeros(nq, np.int32),
                   np.zeros((nq, w), np.uint8), np.zeros((nq, w), np.uint32), np.zeros((nq, w), np.float32),
                   np.zeros((nq, 4), np.float32), [], [])
    for i in range(nq):
        s = int(q_set[i])
        M = np.arange(n) if s < 0 else np.flatnonzero(member[s])
        if len(M) == 0:                                              # an index without docs: nothing anywhere
            empty = np.zeros(0, np.int64)
            out.s_lists.append((empty, empty))
            out.d_lists.append((empty, np.zeros(0, np.float32)))
            continue
        me = -1 if self_ord is None else int(self_ord[i])
        at = np.flatnonzero(M == me)
        sub = fr.fuse(S[i:i + 1, M], D[i:i + 1, M], depth, alpha, np.array([at[0] if len(at) else -1], np.int32))
        c = int(sub.cnt[0])
        out.cnt[i] = c
        out.ords[i, :c] = M[sub.ords[0, :c]]
        for dst, src in ((out.bits, sub.bits), (out.src, sub.src), (out.su, sub.su), (out.de, sub.de)):
            dst[i, :c] = src[0, :c]
        out.rng[i] = sub.rng[0]
        out.s_lists.append((M[sub.s_lists[0][0]], sub.s_lists[0][1]))
        out.d_lists.append((M[sub.d_lists[0][0]], sub.d_lists[0][1]))
    return out
