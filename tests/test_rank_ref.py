"""The numpy rank reference (tests/rank_ref.py) on a hand-computed case, ranks.rank_metrics on hand cases, and its
recall against the reference-shaped recall reporter (recall.RecallMetrics) on a seeded run."""
from types import SimpleNamespace

import numpy as np
import pytest

from mllm_sparse_retrieval_amd.qrels import CrossModalQrels
from mllm_sparse_retrieval_amd.ranks import rank_metrics
from mllm_sparse_retrieval_amd.recall import RECALL_KS, RecallMetrics
from tests import rank_ref

# 6 docs x 3 terms; term 0 sits in every doc (df == N)
D6 = np.array([[1, 2, 0], [1, 0, 3], [1, 2, 0], [1, 0, 0], [1, 5, 0], [1, 0, 1]], dtype=np.int64)
Q_A = [(1, 1), (2, 1), (0, 10), (-1, 4), (1, 0), (2, -3)]   # OOV, zero and negative weights vanish
ALL6 = rank_ref.targets_csr([[0, 1, 2, 3, 4, 5]])


def test_doc_matrix_round_trip():
    assert (rank_ref.doc_matrix(*rank_ref.docs_to_csr(D6), 3) == D6).all()


def test_hand_case_with_df_eq_n_dropped():
    S = rank_ref.scores(*rank_ref.csr([Q_A]), D6, drop_df_eq_n=True)
    assert S.tolist() == [[2, 3, 2, 0, 5, 1]]
    r, s = rank_ref.ranks(S, *ALL6)
    assert r.tolist() == [3, 2, 4, 0, 1, 5]   # docs 0 and 2 tie at 2: the lower ordinal first; doc 3 is no hit
    assert s.tolist() == [2, 3, 2, 0, 5, 1]


def test_hand_case_with_df_eq_n_kept():
    S = rank_ref.scores(*rank_ref.csr([Q_A]), D6, drop_df_eq_n=False)
    assert S.tolist() == [[12, 13, 12, 10, 15, 11]]
    assert rank_ref.ranks(S, *ALL6)[0].tolist() == [3, 2, 4, 6, 1, 5]


def test_hand_case_self_and_duplicates():
    S = rank_ref.scores(*rank_ref.csr([Q_A]), D6)
    r, s = rank_ref.ranks(S, *ALL6, self_ord=[1])
    assert r.tolist() == [2, 0, 3, 0, 1, 4] and s[1] == 3   # self: rank 0, score still reported
    assert rank_ref.ranks(S, *ALL6, self_ord=[-1])[0].tolist() == [3, 2, 4, 0, 1, 5]
    S2 = rank_ref.scores(*rank_ref.csr([[(1, 1), (1, 1)]]), D6)    # duplicate terms add
    assert S2.tolist() == [[4, 0, 4, 0, 10, 0]]
    t = rank_ref.targets_csr([[2, 0, 2, 1]])                       # duplicate targets: the same answer each
    assert rank_ref.ranks(S2, *t)[0].tolist() == [3, 2, 3, 0]


def test_rank_metrics_hand_cases():
    # q0: best 2 (ties in best: 2 twice) | q1: nothing ranked | q2: no targets (not a query of the metric) | q3: best 1
    # q4: best 7
    ranks = [5, 2, 2, 0, 0, 1, 0, 7]
    t_ptr = [0, 3, 5, 5, 6, 8]
    m = rank_metrics(ranks, t_ptr, n_docs=100, ks=[1, 2, 5, 10])
    assert m["n_queries"] == 4 and m["n_unranked"] == 1
    assert m["recall"] == {1: 0.25, 2: 0.5, 5: 0.5, 10: 0.75}
    assert m["mrr"] == pytest.approx((1 / 2 + 0 + 1 + 1 / 7) / 4, rel=0, abs=1e-15)
    assert m["medr"] == (2 + 7) / 2          # best = {2, 101, 1, 7}: even length, the mean of the middle two
    assert m["meanr"] == (2 + 101 + 1 + 7) / 4
    odd = rank_metrics([3, 1, 9], [0, 1, 2, 3], n_docs=10)
    assert odd["medr"] == 3 and odd["recall"][1] == 1 / 3 and set(odd["recall"]) == set(RECALL_KS)
    none = rank_metrics([0, 0], [0, 1, 2], n_docs=10)
    assert none["mrr"] == 0 and none["medr"] == 11 and none["meanr"] == 11 and none["n_unranked"] == 2
    empty = rank_metrics([], [0, 0], n_docs=10)
    assert empty["n_queries"] == 0 and empty["recall"][1] == 0
    with pytest.raises(ValueError):
        rank_metrics([1], [0, 2], n_docs=10)


@pytest.mark.parametrize("query_type", ["text", "image"])
def test_recall_equals_the_recall_reporter(query_type):
    """A seeded run dict: recall[k] of the ranks read off the run equals RecallMetrics' sparse counts / n."""
    rng = np.random.default_rng(5)
    n_images, cpi = 60, 5
    ds = CrossModalQrels.synthetic(n_images, cpi)
    qids = ds.text_id_list if query_type == "text" else ds.img_id_list
    universe = n_images if query_type == "text" else n_images * cpi
    run, ranks, t_ptr = {}, [], [0]
    for qid in qids:
        depth = int(rng.integers(0, 260))
        docs = rng.choice(universe, size=min(depth, universe), replace=False)
        t = ds.get_target(qid, query_type)
        t = [int(x) for x in t] if isinstance(t, list) else [int(t)]
        if rng.random() < 0.3:   # plant a judged doc at the top of some lists, so that r@1 is neither 0 nor 1
            docs = np.concatenate([[t[-1]], docs[docs != t[-1]]])
        sc = np.sort(rng.integers(1, 40, size=len(docs)))[::-1]       # many equal scores: hit order decides
        run[qid] = {"docs": {str(d): float(s) for d, s in zip(docs, sc)}}
        pos = {int(d): i + 1 for i, d in enumerate(docs)}
        ranks.extend(pos.get(x, 0) for x in t)
        t_ptr.append(len(ranks))
    rm = RecallMetrics(ds, {}, run, {}, [], qids, SimpleNamespace(query_type=query_type))
    rm.sort_and_count()
    got = rank_metrics(ranks, t_ptr, universe)
    assert got["n_queries"] == len(qids)
    for k in RECALL_KS:
        assert got["recall"][k] == rm.sparse_counts[k] / len(qids), k
    assert 0 < got["recall"][1] < got["recall"][200] < 1
