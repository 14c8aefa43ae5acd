"""Drop-in for the three pyserini calls the reference makes on its sparse path:

    r = LuceneImpactSearcher(os.path.join(idx, 'index'), None)     src/search.py:273
    r.set_analyzer(JWhiteSpaceAnalyzer())                          src/search.py:274-275
    res = r.batch_search(queries, qids, depth, threads=threads)    src/search.py:86-87
    for hit in res[qid]: hit.score, hit.docid                      src/search.py:96-98

Query handling follows pyserini's behaviour with query_encoder=None as recorded in SURVEY.md §8a A3 ([3P-UNVERIFIED]
there, declared contract here): the query string is split on whitespace and counted (so a token repeated v times has
weight v, src/search.py:419-422), tokens outside the index vocabulary are ignored, tokens present in every doc are
dropped while `min_idf` is 0, and the rest is scored on the GPU by libmsr.so. `threads` is accepted and ignored: the
GPU scores the whole batch at once.
"""
from __future__ import annotations

from collections import Counter

import numpy as np

from ._cabi import MSR_KMAX
from .index import SparseIndex


class JWhiteSpaceAnalyzer:
    """Placeholder for pyserini's analyzer object (src/search.py:274): queries are always whitespace-split here."""


class Hit:
    """One search hit: `docid` is the external id string, `score` a Python float holding the f32 score."""

    __slots__ = ("docid", "score")

    def __init__(self, docid, score):
        self.docid = docid
        self.score = score

    def __repr__(self):
        return f"Hit(docid={self.docid!r}, score={self.score})"


def tokenize_queries(queries):
    """list[str] -> (q_ptr int64, tokens list[str], weights int32): token-frequency encoding, first-seen order."""
    ptr = [0]
    toks, ws = [], []
    for q in queries:
        cnt = Counter(q.split())
        toks.extend(cnt.keys())
        ws.extend(cnt.values())
        ptr.append(len(toks))
    return np.asarray(ptr, dtype=np.int64), toks, np.asarray(ws, dtype=np.int32)


class LuceneImpactSearcher:
    """PARITY UNPINNED for the scorer: T1-T5 below restate pyserini / Lucene impact search as recalled (SURVEY.md §8a
    A3), the reference pins none of it and Lucene cannot run here. The two points most likely to differ from a real
    pyserini run are explicit switches, so an integrator can flip them when checking:
      drop_df_eq_n  None: follow min_idf (terms present in EVERY doc are dropped while min_idf >= 0, contract T3);
                    True / False: force the df == N filter on / off.
      tie rule      a build-time property of the index: `set_build_option("tie_order", 1)` before building numbers the
                    docs in input order (a score tie goes to the doc indexed first, like Lucene's internal doc ids
                    under one indexing thread) instead of doc-id string order (contract T1, the default)."""

    def __init__(self, index_dir, query_encoder=None, min_idf=0, device=0, drop_df_eq_n=None, deep=False):
        if query_encoder is not None:
            raise NotImplementedError("only query_encoder=None (token-frequency queries) is supported, as in the "
                                      "reference (src/search.py:273)")
        self.index = SparseIndex(index_dir, device=device)
        self.min_idf = min_idf
        self.drop_df_eq_n = drop_df_eq_n
        self.deep = bool(deep)  # k > MSR_KMAX goes through SparseIndex.search_deep (up to MSR_DEEP_KMAX)
        self.num_docs = self.index.n_docs

    def set_analyzer(self, analyzer):
        return None

    def close(self):
        self.index.close()

    def _encode(self, queries):
        q_ptr, toks, ws = tokenize_queries(queries)
        return q_ptr, self.index.lookup(toks), ws

    def _idf_rule(self, term_ids, ws):
        """-> (ws, drop_df_eq_n). idf = log(N / df) > min_idf: with the default min_idf = 0 exactly the df == N terms go
        (contract T3, the flag); a positive min_idf is applied here on the host, by zeroing the weights it filters."""
        if self.min_idf > 0:
            df = self.index.df(term_ids).astype(np.float64)
            with np.errstate(divide="ignore"):
                idf = np.log(self.index.n_docs / np.maximum(df, 1e-300))
            ws = np.where((df > 0) & (idf > self.min_idf), ws, 0).astype(np.int32)
            return ws, True if self.drop_df_eq_n is None else bool(self.drop_df_eq_n)
        return ws, self.min_idf >= 0 if self.drop_df_eq_n is None else bool(self.drop_df_eq_n)

    def search(self, q, k=10):
        return self.batch_search([q], ["_q"], k)["_q"]

    def batch_search(self, queries, qids, k=10, threads=1, fields=None):
        if len(queries) != len(qids):
            raise ValueError("queries and qids differ in length")
        # a positive min_idf needs the term ids on this side (Python tokenisation), everything else tokenises in C
        if self.deep and k > MSR_KMAX:
            if self.min_idf > 0:
                q_ptr, term_ids, ws = self._encode(queries)
                ws, drop = self._idf_rule(term_ids, ws)
            else:
                q_ptr, term_ids, ws = self.index.encode_queries(queries)
                drop = self._idf_rule(None, None)[1]
            ords, scores, _, n = self.index.search_deep(q_ptr, term_ids, ws, k, drop_df_eq_n=drop)
        elif self.min_idf > 0:
            q_ptr, term_ids, ws = self._encode(queries)
            ws, drop = self._idf_rule(term_ids, ws)
            ords, scores, _, n = self.index.search_csr(q_ptr, term_ids, ws, k, drop_df_eq_n=drop)
        else:
            ords, scores, _, n = self.index.search_text(queries, k, drop_df_eq_n=self._idf_rule(None, None)[1])
        out = {}
        table = self.index.docid_table() if len(qids) * k > 64 else None
        score_rows = scores.tolist()
        for i, qid in enumerate(qids):  # duplicate qids collapse, like the qid-keyed map pyserini returns
            cnt = int(n[i])
            ids = table[ords[i, :cnt]].tolist() if table is not None else self.index.docids(ords[i, :cnt])
            row = score_rows[i]
            out[qid] = [Hit(ids[j], row[j]) for j in range(cnt)]
        return out

    def batch_search_filtered(self, queries, qids, k, doc_sets, query_set):
        """batch_search among named doc sets (SparseIndex.search_filtered): doc_sets maps a set name to external doc ids,
        query_set maps a qid to the name of its set; a qid without an entry is unfiltered. Returns {qid: [Hit, ...]} like
        batch_search (duplicate qids collapse). A doc id the index does not hold, or a set name doc_sets does not have,
        is a ValueError; a doc that is listed in no set belongs to no set. Counterpart: a Lucene filter query, which
        pyserini's batch_search does not take."""
        from .filters import sets_from_ordinals

        if len(queries) != len(qids):
            raise ValueError("queries and qids differ in length")
        if getattr(self, "_ord_of", None) is None:
            self._ord_of = {d: o for o, d in enumerate(self.index.docid_table().tolist())}
        ord_of = self._ord_of
        names = list(doc_sets)
        col = {name: s for s, name in enumerate(names)}
        lists = []
        for name in names:
            unknown = [str(d) for d in doc_sets[name] if str(d) not in ord_of]
            if unknown:
                raise ValueError(f"doc set {name!r}: the index does not hold doc id {unknown[0]!r}"
                                 + (f" (and {len(unknown) - 1} more)" if len(unknown) > 1 else ""))
            lists.append([ord_of[str(d)] for d in doc_sets[name]])
        q_set = np.full(len(qids), -1, dtype=np.int32)
        for i, qid in enumerate(qids):
            name = query_set.get(qid)
            if name is None:
                continue
            if name not in col:
                raise ValueError(f"query {qid!r} names doc set {name!r}, which doc_sets does not have")
            q_set[i] = col[name]
        if self.min_idf > 0:
            q_ptr, term_ids, ws = self._encode(queries)
        else:
            q_ptr, term_ids, ws = self.index.encode_queries(queries)
        ws, drop = self._idf_rule(term_ids, ws)
        bits = sets_from_ordinals(lists, self.index.n_docs)
        ords, scores, _, n = self.index.search_filtered(q_ptr, term_ids, ws, k, bits, q_set, drop_df_eq_n=drop)
        out = {}
        table = self.index.docid_table()
        score_rows = scores.tolist()
        for i, qid in enumerate(qids):
            cnt = int(n[i])
            ids = table[ords[i, :cnt]].tolist()
            row = score_rows[i]
            out[qid] = [Hit(ids[j], row[j]) for j in range(cnt)]
        return out

    def batch_rank(self, queries, qids, targets, remove_query=False):
        """Exact rank and score of named docs: targets[i] lists external doc ids for queries[i]. Returns
        {qid: [(docid, rank, score), ...]} in the given order; rank 0 = not a hit (score 0) or, with remove_query, the
        query's own doc; an id the index does not hold comes back as (docid, None, None). No pyserini counterpart: a
        hit list stops at its depth (src/search.py:86-99), these ranks do not (SparseIndex.rank_docs)."""
        if not (len(queries) == len(qids) == len(targets)):
            raise ValueError("queries, qids and targets differ in length")
        table = self.index.docid_table()
        if getattr(self, "_ord_of", None) is None:
            self._ord_of = {d: o for o, d in enumerate(table.tolist())}
        ord_of = self._ord_of
        q_ptr, term_ids, ws = self._encode(queries) if self.min_idf > 0 else self.index.encode_queries(queries)
        ws, drop = self._idf_rule(term_ids, ws)
        t_ptr, t_ord = [0], []
        for tg in targets:
            t_ord.extend(ord_of[str(d)] for d in tg if str(d) in ord_of)
            t_ptr.append(len(t_ord))
        self_ord = np.asarray([ord_of.get(str(x), -1) for x in qids], dtype=np.int32) if remove_query else None
        ranks, scores = self.index.rank_docs(q_ptr, term_ids, ws, np.asarray(t_ptr, np.int64), np.asarray(t_ord, np.uint32),
                                             drop_df_eq_n=drop, self_ord=self_ord)
        ranks, scores = ranks.tolist(), scores.tolist()
        out = {}
        for i, qid in enumerate(qids):
            e = t_ptr[i]
            row = []
            for d in targets[i]:
                if str(d) in ord_of:
                    row.append((d, ranks[e], scores[e]))
                    e += 1
                else:
                    row.append((d, None, None))
            out[qid] = row
        return out

    def batch_explain(self, queries, qids, targets):
        """Why named docs score what they score: targets[i] lists external doc ids for queries[i] (at most
        MSR_EXPLAIN_MAX_TARGETS known ids each). Returns {qid: [(docid, score, rows), ...]} in the given order, rows =
        [(token, q_w, d_w, q_w * d_w), ...] for the query tokens the doc holds (contribution descending, then token
        bytewise; explain.rows_of) and score = their sum, the exact score batch_rank reports; an id the index does not
        hold comes back as (docid, None, None). Counterpart: Lucene's explain(), which the reference never calls
        (SparseIndex.explain_docs)."""
        from .explain import build_rows, score_of

        if not (len(queries) == len(qids) == len(targets)):
            raise ValueError("queries, qids and targets differ in length")
        table = self.index.docid_table()
        if getattr(self, "_ord_of", None) is None:
            self._ord_of = {d: o for o, d in enumerate(table.tolist())}
        ord_of = self._ord_of
        q_ptr, toks, ws = tokenize_queries(queries)  # (the tokens name the rows, so they are kept on this side)
        term_ids = self.index.lookup(toks)
        ws, drop = self._idf_rule(term_ids, ws)
        t_ptr, t_ord = [0], []
        for tg in targets:
            t_ord.extend(ord_of[str(d)] for d in tg if str(d) in ord_of)
            t_ptr.append(len(t_ord))
        x_ptr, doc_w = self.index.explain_docs(q_ptr, term_ids, ws, np.asarray(t_ptr, np.int64),
                                               np.asarray(t_ord, np.uint32), drop_df_eq_n=drop)
        rows = build_rows(q_ptr, toks, ws.tolist(), t_ptr, x_ptr, doc_w.tolist())
        out = {}
        for i, qid in enumerate(qids):
            e = t_ptr[i]
            row = []
            for d in targets[i]:
                if str(d) in ord_of:
                    row.append((d, score_of(rows[e]), rows[e]))
                    e += 1
                else:
                    row.append((d, None, None))
            out[qid] = row
        return out

    def _ords_of(self, docids):
        """External doc ids -> (known ids as strings in the given order, their ordinals uint32)."""
        if getattr(self, "_ord_of", None) is None:
            self._ord_of = {d: o for o, d in enumerate(self.index.docid_table().tolist())}
        known = [str(d) for d in docids if str(d) in self._ord_of]
        return known, np.asarray([self._ord_of[d] for d in known], dtype=np.uint32)

    def batch_doc_vectors(self, docids):
        """What named docs hold: {docid: {token: weight}} with the tokens in ascending term id, None for an id the index
        does not hold. Counterpart: pyserini's IndexReader.get_document_vector(docid), which the reference never calls;
        the vectors are read out of the inverted index on the GPU (SparseIndex.doc_vectors)."""
        known, ords = self._ords_of(docids)
        d_ptr, term, weight = self.index.doc_vectors(ords)
        toks = {t: self.index.term_str(t) for t in np.unique(term).tolist()}
        d_ptr, term, weight = d_ptr.tolist(), term.tolist(), weight.tolist()
        by_str = {}
        for e, d in enumerate(known):
            by_str[d] = {toks[term[j]]: weight[j] for j in range(d_ptr[e], d_ptr[e + 1])}
        return {d: by_str.get(str(d)) for d in docids}

    def batch_search_docs(self, docids, k=10, remove_self=True):
        """Search with docs of the index as the queries: {docid: [Hit, ...]}, None for an id the index does not hold.
        The query of a doc is its stored vector (its terms, its weights as query weights), under the searcher's own
        drop_df_eq_n / min_idf rule; MSR_E_OVERFLOW / MSR_E_RANGE refusals of the search are passed on. With remove_self
        the search runs at k + 1 and the doc itself is dropped (so k <= MSR_KMAX - 1). Host glue over
        SparseIndex.doc_vectors and search_csr."""
        depth = k + 1 if remove_self else k
        if k < 1 or depth > MSR_KMAX:
            raise ValueError(f"k = {k} is outside 1 .. {MSR_KMAX - 1 if remove_self else MSR_KMAX}"
                             + (" (remove_self searches at k + 1)" if remove_self else ""))
        known, ords = self._ords_of(docids)
        if not known:
            return {d: None for d in docids}
        d_ptr, term, weight = self.index.doc_vectors(ords)
        term_ids, ws = term.astype(np.int32), weight.astype(np.int32)
        ws, drop = self._idf_rule(term_ids, ws)
        res_ord, scores, _, n = self.index.search_csr(d_ptr, term_ids, ws, depth, drop_df_eq_n=drop)
        table = self.index.docid_table()
        by_str = {}
        for i, d in enumerate(known):
            cnt = int(n[i])
            row_o, row_s = res_ord[i, :cnt], scores[i, :cnt].tolist()
            keep = [j for j in range(cnt) if not (remove_self and int(row_o[j]) == int(ords[i]))][:k]
            ids = table[row_o].tolist()
            by_str[d] = [Hit(ids[j], row_s[j]) for j in keep]
        return {d: by_str.get(str(d)) for d in docids}
