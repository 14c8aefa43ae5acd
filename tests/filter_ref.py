"""numpy reference for the filtered searches (msr_search_filtered, msr_dense_search_filtered; include/msr.h): the bit
packing of doc sets, the masked top-k and the named sets the GPU tests use. Built on tests/rank_ref.py (S = Q @ D.T) and
tests/deep_ref.py (topk_rows); nothing here calls libmsr, every comparison against it is exact equality.

    member  bool [n_sets, n]                 doc o belongs to set s
    words   uint32 [n_sets, (n + 31) // 32]  bit (o & 31) of word (o >> 5) of row s  (bit 0 = LSB)
    q_set   int [nq] in [-1, n_sets)         -1: the query is unfiltered

The filtered list of query i is dr.topk_rows((K * mask)[i], k) with mask[i] = member[q_set[i]] (all ones for -1) and K
the matrix of u32 keys (sparse: exact scores, 0 = no hit; dense: the order-preserving key of the f32 score, never 0 for
a finite score), i.e. the unfiltered exact ranking with the non-members struck out, cut to k."""
from __future__ import annotations

import numpy as np

from tests import deep_ref as dr


def words_of(n):
    return (n + 31) // 32


def pack(member):
    """bool [n_sets, n] -> uint32 [n_sets, W], by shifts and adds (not by np.packbits, which the package uses)."""
    member = np.atleast_2d(np.asarray(member, dtype=bool))
    n_sets, n = member.shape
    w = words_of(n)
    out = np.zeros((n_sets, w), dtype=np.uint64)
    cols = np.arange(n)
    for s in range(n_sets):
        np.add.at(out[s], cols[member[s]] >> 5, np.uint64(1) << (cols[member[s]] & 31).astype(np.uint64))
    return out.astype(np.uint32)


def unpack(words, n):
    """uint32 [n_sets, W] -> bool [n_sets, n]; bits at or above n are ignored."""
    words = np.atleast_2d(np.asarray(words, dtype=np.uint32))
    cols = np.arange(n)
    return ((words[:, cols >> 5] >> (cols & 31).astype(np.uint32)) & 1).astype(bool)


def mask_rows(member, q_set, nq):
    """bool [nq, n]: row i = member[q_set[i]], all ones where q_set[i] == -1 (q_set None: set 0 for everyone when there
    is one set, unfiltered when there is none)."""
    member = np.asarray(member, dtype=bool)
    n = member.shape[1]
    if q_set is None:
        assert member.shape[0] <= 1
        q_set = np.full(nq, 0 if member.shape[0] == 1 else -1)
    q_set = np.asarray(q_set, dtype=np.int64)
    assert q_set.shape == (nq,) and q_set.min(initial=0) >= -1 and q_set.max(initial=-1) < member.shape[0]
    out = np.ones((nq, n), dtype=bool)
    pick = q_set >= 0
    out[pick] = member[q_set[pick]]
    return out


def masked_topk(K, member, q_set, k):
    """-> (cols uint32 [nq, k], keys uint32 [nq, k], n_hit int32 [nq]) of the filtered search over the key matrix K."""
    K = np.asarray(K)
    return dr.topk_rows(K.astype(np.int64) * mask_rows(member, q_set, K.shape[0]), k)


def cut(ref, k):
    """The reference at depth k from the reference at a depth >= k (a top-k list is a prefix of every deeper one)."""
    idx, keys, n_hit = ref
    assert k <= idx.shape[1]
    return idx[:, :k].copy(), keys[:, :k].copy(), np.minimum(n_hit, k).astype(np.int32)


SET_NAMES = ("empty", "full", "last", "tile1", "even", "span", "random", "full_garbage")


def named_sets(n, tile, seed=9):
    """The eight sets of the GPU tests over n docs with tiles of `tile` docs -> (member bool [8, n], words uint32 [8, W]):
    empty; full; only doc n - 1; exactly tile 1 (tiles 0 and 2 hold no member); every even ordinal; [5, tile + 3), whose
    edges are off the 4- and 32-doc grid and cross a tile; random p = 0.5; full with garbage bits set above n in the last
    word (member row = full: those bits name no doc)."""
    assert n > tile + 3 and n % 32 != 0
    o = np.arange(n)
    member = np.zeros((len(SET_NAMES), n), dtype=bool)
    member[1] = True
    member[2, n - 1] = True
    member[3] = (o >= tile) & (o < 2 * tile)
    member[4] = o % 2 == 0
    member[5] = (o >= 5) & (o < tile + 3)
    member[6] = np.random.default_rng(seed).random(n) < 0.5
    member[7] = True
    words = pack(member)
    words[7, -1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
    return member, words


def cut_rows(K, mask, k):
    """Rows of the masked key matrix whose k-th place falls inside a tie class (dr.tie_class: some but not all of the
    members with the k-th key are taken)."""
    out = []
    for i in range(K.shape[0]):
        _, cls, taken = dr.tie_class(np.asarray(K[i]).astype(np.int64) * mask[i], k)
        if 0 < taken < cls:
            out.append(i)
    return out
