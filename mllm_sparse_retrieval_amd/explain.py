"""Readable scores from SparseIndex.explain_docs: which tokens carry a (query, doc) match and by how much.

A learned-sparse score is a sum of `query weight x doc weight` over vocabulary tokens. explain_docs returns the stored
doc weight of every query entry for listed docs; this module turns that ragged array into rows
(token, q_w, d_w, q_w * d_w) per listed doc and writes them as TSV. Counterpart: Lucene's explain(); the reference has
none on its search path (src/search.py) and inspects the encoder output instead (src/sparse_statistic.py).
"""
from __future__ import annotations


def _token_key(tok):
    return tok if isinstance(tok, bytes) else str(tok).encode("utf-8", "surrogateescape")


def rows_of(tokens, q_w, d_w):
    """One listed doc: parallel sequences over the query's entries -> [(token, q_w, d_w, q_w * d_w), ...] for the
    entries the doc matches (d_w > 0; an entry that does not count comes with d_w == 0). Entries of one token are merged
    (their query weights add, as in the score). Sorted by contribution descending, then by token bytewise."""
    merged = {}
    for tok, qw, dw in zip(tokens, q_w, d_w):
        qw, dw = int(qw), int(dw)
        if dw <= 0 or qw <= 0:
            continue
        if tok in merged:
            merged[tok][0] += qw
        else:
            merged[tok] = [qw, dw]
    rows = [(tok, qw, dw, qw * dw) for tok, (qw, dw) in merged.items()]
    rows.sort(key=lambda r: (-r[3], _token_key(r[0])))
    return rows


def build_rows(q_ptr, tokens, q_w, t_ptr, x_ptr, doc_w):
    """The CSR handed to explain_docs (tokens: one string per query entry) and its result -> one row list per target
    entry, in t_ord order."""
    out = []
    for i in range(len(q_ptr) - 1):
        b, e = int(q_ptr[i]), int(q_ptr[i + 1])
        for t in range(int(t_ptr[i]), int(t_ptr[i + 1])):
            x = int(x_ptr[t])
            if int(x_ptr[t + 1]) - x != e - b:
                raise ValueError("x_ptr does not match the query CSR")
            out.append(rows_of(tokens[b:e], q_w[b:e], doc_w[x:x + e - b]))
    return out


def score_of(rows):
    return sum(r[3] for r in rows)


TSV_COLUMNS = ("qid", "docid", "position", "judged", "score", "token", "q_w", "d_w", "contribution")


def tsv_lines(records):
    """records: (qid, docid, position, judged, rows) -> one line per matched token:
    qid, docid, position (1-based place among the returned hits, 0 = not returned), judged (0/1), score, token, q_w,
    d_w, contribution. A listed doc with score 0 gets one line with token `-` and zeros."""
    for qid, docid, position, judged, rows in records:
        head = f"{qid}\t{docid}\t{int(position)}\t{1 if judged else 0}\t{score_of(rows)}"
        if not rows:
            yield head + "\t-\t0\t0\t0\n"
        for tok, qw, dw, c in rows:
            yield f"{head}\t{tok}\t{qw}\t{dw}\t{c}\n"


def write_tsv(path, records):
    with open(path, "w", encoding="utf-8", errors="surrogateescape") as f:
        f.writelines(tsv_lines(records))
