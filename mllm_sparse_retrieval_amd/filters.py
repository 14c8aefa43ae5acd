"""Doc sets of the filtered searches (msr_search_filtered / msr_dense_search_filtered, include/msr.h).

A set is a row of a bitmap over doc ordinals (sparse route) or rows (dense route): bit (o & 31) (bit 0 = LSB) of word
(o >> 5) says that doc o is a member. The helpers here build such bitmaps and read the two TSV files of the command
line (search --doc_sets FILE --query_sets FILE): lines `docid<TAB>set` and `qid<TAB>set`.
"""
from __future__ import annotations

import numpy as np

MSR_FILTER_MAX_SETS = 65536


def set_words(n):
    """uint32 words of one bitmap row over n docs."""
    return (int(n) + 31) // 32


def pack_doc_sets(bool_matrix):
    """bool [n_sets, n] (or [n] for one set) -> packed uint32 [n_sets, (n + 31) // 32], bit 0 of word 0 = doc 0."""
    m = np.asarray(bool_matrix)
    if m.ndim == 1:
        m = m[None, :]
    if m.ndim != 2:
        raise ValueError("expected a [n_sets, n] membership matrix")
    m = m.astype(bool)
    n_sets, n = m.shape
    w = set_words(n)
    padded = np.zeros((n_sets, w * 32), dtype=np.uint8)
    padded[:, :n] = m
    by = np.packbits(padded, axis=1, bitorder="little")          # [n_sets, 4 w] bytes, little-endian bit order
    return np.ascontiguousarray(by).view("<u4").astype(np.uint32).reshape(n_sets, w)


def unpack_doc_sets(packed, n):
    """Inverse of pack_doc_sets: packed uint32 [n_sets, W] -> bool [n_sets, n] (bits at or above n are dropped)."""
    p = np.ascontiguousarray(packed, dtype=np.uint32)
    if p.ndim != 2 or p.shape[1] != set_words(n):
        raise ValueError(f"expected [n_sets, {set_words(n)}] words for {n} docs, got shape {p.shape}")
    bits = np.unpackbits(p.astype("<u4").view(np.uint8).reshape(p.shape[0], -1), axis=1, bitorder="little")
    return bits[:, :n].astype(bool)


def sets_from_ordinals(lists, n):
    """One list of doc ordinals (or rows) per set -> packed uint32 [n_sets, W]; an ordinal outside [0, n) is an error."""
    m = np.zeros((len(lists), int(n)), dtype=bool)
    for s, ords in enumerate(lists):
        o = np.asarray(ords, dtype=np.int64).reshape(-1)
        if o.size and (o.min() < 0 or o.max() >= n):
            raise ValueError(f"set {s}: ordinal outside [0, {n})")
        m[s, o] = True
    return pack_doc_sets(m)


def as_packed_sets(sets, n):
    """What the search_filtered methods accept: a bool [n_sets, n] matrix or packed uint32 [n_sets, W] -> packed."""
    a = np.asarray(sets)
    if a.dtype == bool:
        if a.ndim == 1:
            a = a[None, :]
        if a.ndim != 2 or a.shape[1] != n:
            raise ValueError(f"bool doc sets need shape [n_sets, {n}], got {a.shape}")
        return pack_doc_sets(a)
    if a.dtype != np.uint32:
        raise ValueError("doc sets are a bool [n_sets, n] matrix or packed uint32 words (pack_doc_sets)")
    if a.ndim == 1 and a.size == set_words(n):
        a = a[None, :]
    if a.ndim != 2 or a.shape[1] != set_words(n):
        raise ValueError(f"packed doc sets need shape [n_sets, {set_words(n)}] for {n} docs, got {a.shape}")
    return np.ascontiguousarray(a)


def as_q_set(q_set, nq, n_sets):
    """q_set argument -> int32 [nq] or None (allowed for 0 or 1 sets: nothing filtered / every query uses set 0)."""
    if q_set is None:
        if n_sets > 1:
            raise ValueError("q_set is required with more than one doc set")
        return None
    q = np.ascontiguousarray(q_set, dtype=np.int32)
    if q.shape != (nq,):
        raise ValueError(f"q_set needs one entry per query ({nq}), got shape {q.shape}")
    return q


def _read_pairs(path, what):
    out = []
    with open(path, "r", encoding="utf-8") as f:
        for ln, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            if not line.strip():
                continue
            parts = line.split("\t")
            if len(parts) != 2 or not parts[0] or not parts[1]:
                raise ValueError(f"{path}:{ln}: expected `{what}<TAB>set`, got {line!r}")
            out.append((parts[0], parts[1]))
    return out


def read_doc_sets(path):
    """TSV lines `docid<TAB>set` -> {set name: [docid, ...]} in file order (a doc may be in several sets)."""
    sets = {}
    for docid, name in _read_pairs(path, "docid"):
        sets.setdefault(name, []).append(docid)
    return sets


def read_query_sets(path):
    """TSV lines `qid<TAB>set` -> {qid: set name}; a qid listed twice with different sets is an error."""
    out = {}
    for qid, name in _read_pairs(path, "qid"):
        if out.setdefault(qid, name) != name:
            raise ValueError(f"{path}: query {qid!r} is assigned to both {out[qid]!r} and {name!r}")
    return out
