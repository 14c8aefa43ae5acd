"""Hybrid fusion and TREC run files — the reference's src/hybrid.py:8-90 semantics.

fuse(): for every doc in the union of the runs' result lists, sum over runs of
    weight * (score - min_score) / max(max_score - min_score, 1e-9)   if the run retrieved the doc, else 0,
with min/max as recorded by get_run_dict (over the unfiltered list). Output {qid: {doc: fused score}} (no 'docs' level).
"""
from __future__ import annotations


def fuse(runs, weights):
    """src/hybrid.py:32-53."""
    qids = set()
    for run in runs:
        qids.update(run)
    fused = {}
    for qid in qids:
        acc = {}
        spans = [(r[qid]["min_score"], max(r[qid]["max_score"] - r[qid]["min_score"], 1e-9)) for r in runs]
        for run in runs:
            for doc in run[qid]["docs"]:
                if doc in acc:
                    continue
                total = 0
                for other, weight, (lo, den) in zip(runs, weights, spans):
                    s = other[qid]["docs"].get(doc)
                    if s is not None:
                        total += weight * ((s - lo) / den)
                acc[doc] = total
        fused[qid] = acc
    return fused


class ResultRecord:
    """src/hybrid.py:3-6: a fused score and where it came from ('dense', 'sparse' or 'fuse' = both lists held the doc)."""

    __slots__ = ("score", "type")

    def __init__(self, score, type):
        self.score = score
        self.type = type

    def __repr__(self):
        return f"ResultRecord(score={self.score}, type={self.type!r})"


def fuse_statistic(runs, weights):
    """src/hybrid.py:56-90 (used by the reference's score_statistic.py): fuse() that also says which run(s) a doc's
    score came from. A doc found in exactly one run is tagged by the POSITION of the run being walked when the doc is
    first met ('dense' while walking runs[0], 'sparse' afterwards), as the reference does; found in more: 'fuse'."""
    qids = set()
    for run in runs:
        qids.update(run)
    fused = {}
    for qid in qids:
        acc = {}
        spans = [(r[qid]["min_score"], max(r[qid]["max_score"] - r[qid]["min_score"], 1e-9)) for r in runs]
        for position, run in enumerate(runs, start=1):
            for doc in run[qid]["docs"]:
                if doc in acc:
                    continue
                total, found = 0, 0
                for other, weight, (lo, den) in zip(runs, weights, spans):
                    s = other[qid]["docs"].get(doc)
                    if s is not None:
                        total += weight * ((s - lo) / den)
                        found += 1
                kind = ("dense" if position == 1 else "sparse") if found == 1 else "fuse"
                acc[doc] = ResultRecord(total, kind)
        fused[qid] = acc
    return fused


_SRC_TYPES = (None, "dense", "sparse", "fuse")  # out_src of msr_hybrid_search_union -> ResultRecord.type


def _list_run(qids, names, member, key, scores, lo, hi, empty):
    """One depth list per query out of the union arrays: the members flagged by `member`, ordered by `key` ascending
    (a composite of descending score and ascending ordinal), as {'docs': {doc: score}, 'min_score', 'max_score'}."""
    import numpy as np

    big = np.uint64(0xFFFFFFFFFFFFFFFF)  # (no member's key: the ordinal half stays below 2^32 - 1)
    order = np.argsort(np.where(member, key, big), axis=1, kind="stable")
    cnt = member.sum(axis=1)
    docs = np.take_along_axis(names, order, axis=1)
    vals = np.take_along_axis(scores, order, axis=1)
    run = {}
    for i, qid in enumerate(qids):
        c = int(cnt[i])
        v = vals[i, :c]
        run[qid] = {"docs": dict(zip(docs[i, :c].tolist(), v.tolist() if v.dtype != np.float32 else v)),
                    "min_score": 0 if empty[i] else lo[i], "max_score": 0 if empty[i] else hi[i]}
    return run


def union_to_runs(qids, docid_table, ords, n, fused, src=None, sparse_u32=None, dense=None, score_range=None):
    """The arrays of dense.hybrid_search_union -> (sparse_run, dense_run, fusion_run) in the layouts of get_run_dict
    (src/search.py:66-82) and fuse (src/hybrid.py:32-53): the two lists as {'docs': {doc: score}, 'min_score',
    'max_score'} with docs best first (score ties: lower ordinal, in both lists) and min / max from score_range, i.e. over
    the UNFILTERED list as get_run_dict takes them; the fused run as {qid: {doc: score}} best first. Sparse and fused
    scores are Python floats of the f32 values, dense scores numpy float32, as the other GPU route builds them.
    docid_table: ordinal -> external id (SparseIndex.docid_table()). Without the four list arrays (a with_lists=False
    call) the two list runs come back empty and only the fused run is built."""
    import numpy as np

    ords, n = np.asarray(ords), np.asarray(n)
    nq, w = ords.shape
    if n.shape != (nq,) or len(qids) != nq:
        raise ValueError(f"expected one member count and one query id per row of ords ({nq}), got n of shape {n.shape} "
                         f"and {len(qids)} ids")
    live = np.arange(w)[None, :] < n[:, None]
    table = np.asarray(docid_table, dtype=object)
    names = table[np.where(live, ords, 0)] if len(table) else np.empty((nq, w), dtype=object)
    fused_rows = np.asarray(fused, dtype=np.float32)
    fusion_run = {qid: dict(zip(names[i, :n[i]].tolist(), fused_rows[i, :n[i]].tolist())) for i, qid in enumerate(qids)}
    if src is None:
        return {}, {}, fusion_run
    src = np.asarray(src)
    o64 = ords.astype(np.uint64)
    s_u32 = np.asarray(sparse_u32, dtype=np.uint32)
    d_f32 = np.ascontiguousarray(dense, dtype=np.float32)
    bits = d_f32.view(np.uint32)
    d_key = np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint64)  # order-preserving
    rng = np.asarray(score_range, dtype=np.float32)
    sparse_run = _list_run(qids, names, live & ((src & 2) != 0), ((np.uint64(0xFFFFFFFF) - s_u32.astype(np.uint64)) << np.uint64(32)) | o64,
                           s_u32.astype(np.float32).astype(np.float64), rng[:, 3].tolist(), rng[:, 2].tolist(),
                           rng[:, 2] == 0)
    dense_run = _list_run(qids, names, live & ((src & 1) != 0), ((np.uint64(0xFFFFFFFF) - d_key) << np.uint64(32)) | o64, d_f32,
                          rng[:, 1], rng[:, 0], np.zeros(nq, dtype=bool) if len(table) else np.ones(nq, dtype=bool))
    return sparse_run, dense_run, fusion_run


def union_to_statistic(qids, docid_table, ords, n, fused, src):
    """The arrays of dense.hybrid_search_union -> {qid: {doc: ResultRecord}} as fuse_statistic([dense, sparse], ...)
    returns it (src/hybrid.py:56-90): the fused score and 'dense' / 'sparse' / 'fuse' for where it came from."""
    import numpy as np

    ords, n, src = np.asarray(ords), np.asarray(n), np.asarray(src)
    table = np.asarray(docid_table, dtype=object)
    fused_rows = np.asarray(fused, dtype=np.float32)
    out = {}
    for i, qid in enumerate(qids):
        c = int(n[i])
        out[qid] = {d: ResultRecord(s, _SRC_TYPES[t & 3]) for d, s, t in
                    zip(table[ords[i, :c]].tolist(), fused_rows[i, :c].tolist(), src[i, :c].tolist())}
    return out


def write_trec_run(run, file, name="fusion"):
    """src/hybrid.py:20-29: `qid Q0 doc rank score name`, docs by score descending (stable)."""
    with open(file, "w") as f:
        for qid, entry in run.items():
            docs = entry["docs"] if "docs" in entry else entry
            ranked = sorted(docs.items(), key=lambda kv: kv[1], reverse=True)
            for rank, (doc, score) in enumerate(ranked, start=1):
                f.write(f"{qid} Q0 {doc} {rank} {score} {name}\n")


def read_trec_run(file):
    """src/hybrid.py:8-17: max_score is the first line's score of a qid, min_score the last line's."""
    run = {}
    with open(file, "r") as f:
        for line in f:
            qid, _, docid, _rank, score, _ = line.strip().split()
            score = float(score)
            if qid not in run:
                run[qid] = {"docs": {}, "max_score": score, "min_score": score}
            run[qid]["docs"][docid] = score
            run[qid]["min_score"] = score
    return run
