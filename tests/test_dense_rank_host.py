"""msr_dense_rank_rows without a GPU: the numpy reference (tests/dense_rank_ref.py) on a hand-written key matrix and
against f32_chain.topk, the null-handle refusal through ctypes, and the CLI checks of search --ranks on the dense route."""
import ctypes

import numpy as np
import pytest

from tests.dense_rank_ref import ranks_from_keys, targets_csr
from tests.f32_chain import chain_scores, f32_keys, topk

INVAL = -1


@pytest.fixture(scope="module")
def m(built):
    import mllm_sparse_retrieval_amd as m

    return m


def test_reference_on_a_hand_written_matrix():
    # query 0: rows 1 and 2 tie (70), row 4 is the best; query 1 lists nothing
    keys = np.array([[50, 70, 70, 30, 90, 10],
                     [5, 5, 9, 1, 7, 3]], dtype=np.uint32)
    # listed: the tie pair, the upper twin again, row 0 (the self row below), two rows the self row beats
    t_ptr, t_row = targets_csr([[1, 2, 2, 0, 3, 5], []])
    r, k = ranks_from_keys(keys, t_ptr, t_row, None)
    assert k.tolist() == [70, 70, 70, 50, 30, 10]
    assert r.tolist() == [2, 3, 3, 4, 5, 6]
    # self = row 0 (key 50): below the tie pair (their ranks stay), above rows 3 and 5 (they move up one), itself rank 0
    r, k = ranks_from_keys(keys, t_ptr, t_row, np.array([0, -1]))
    assert k.tolist() == [70, 70, 70, 50, 30, 10]
    assert r.tolist() == [2, 3, 3, 0, 4, 5]
    # self = the best row: everything moves up one; self = the lower twin: only the upper twin and what lies below move
    assert ranks_from_keys(keys, t_ptr, t_row, np.array([4, 2]))[0].tolist() == [1, 2, 2, 3, 4, 5]
    assert ranks_from_keys(keys, t_ptr, t_row, np.array([1, -1]))[0].tolist() == [0, 2, 2, 3, 4, 5]
    assert ranks_from_keys(keys, t_ptr, t_row, np.array([2, -1]))[0].tolist() == [2, 0, 0, 3, 4, 5]
    # the second query's row: ties to the lower row, nothing is "not ranked"
    t_ptr, t_row = targets_csr([[], [1, 0, 3]])
    assert ranks_from_keys(keys, t_ptr, t_row, None)[0].tolist() == [4, 3, 6]


def test_reference_agrees_with_the_topk_reference():
    rng = np.random.default_rng(12)
    p = rng.standard_normal((40, 7)).astype(np.float32)
    p[13::13] = p[0]  # ties
    p[5] = -p[5]
    q = rng.standard_normal((5, 7)).astype(np.float32)
    q[4] = 0          # every score +0: one tie over the whole row, broken by the row index
    scores = chain_scores(q, p)
    t_ptr, t_row = targets_csr([list(range(40))] * 5)
    ranks, keys = ranks_from_keys(f32_keys(scores), t_ptr, t_row, None)
    ranks, keys = ranks.reshape(5, 40), keys.reshape(5, 40)
    assert (np.sort(ranks, axis=1) == np.arange(1, 41)).all()  # a permutation: ties are broken, nobody is unranked
    for k in (1, 10, 40, 50):
        idx, key, n = topk(scores, k)
        for i in range(5):
            for t in range(40):
                if ranks[i, t] <= k:
                    assert idx[i, ranks[i, t] - 1] == t and key[i, ranks[i, t] - 1] == keys[i, t]
                else:
                    assert t not in idx[i, :n[i]]


def test_null_handle_is_refused(m):
    from mllm_sparse_retrieval_amd import _cabi

    assert hasattr(ctypes.CDLL(_cabi.LIB_PATH), "msr_dense_rank_rows")
    assert _cabi.MSR_DENSE_RANK_MAX_TARGETS == 64
    q = np.zeros((1, 4), np.float32)
    t_ptr, t_row = targets_csr([[0]])
    out = np.zeros(1, np.uint32)
    p = _cabi.ptr
    rc = _cabi.lib().msr_dense_rank_rows(None, p(q), 1, 1, p(t_ptr), p(t_row), None, p(out), p(out), None)
    assert rc == INVAL and b"msr_dense_rank_rows" in _cabi.lib().msr_last_error()


def test_cli_dense_ranks_needs_qrels(m):
    from mllm_sparse_retrieval_amd import cli

    with pytest.raises(SystemExit) as e:
        cli.main(["search", "--passage_reps", "nowhere", "--ranks"])
    assert isinstance(e.value.code, str) and "--ranks" in e.value.code and "--qrels" in e.value.code


def test_cli_dense_ranks_refused_under_a_launcher(m, monkeypatch):
    from mllm_sparse_retrieval_amd import cli

    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        cli.main(["search", "--passage_reps", "nowhere", "--qrels", "q.csv", "--ranks"])
    assert isinstance(e.value.code, str) and "WORLD_SIZE" in e.value.code


def test_cli_help_names_the_dense_route(m, capsys):
    from mllm_sparse_retrieval_amd import cli

    with pytest.raises(SystemExit) as e:
        cli.main(["search", "--help"])
    assert e.value.code == 0
    text = " ".join(capsys.readouterr().out.split())
    assert "msr_dense_rank_rows" in text and "dense.ranks.tsv" in text
