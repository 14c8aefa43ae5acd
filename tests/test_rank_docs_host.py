"""msr_rank_docs without a GPU: the symbol, every argument refusal (they come before the device is looked at), the
no-device refusal of a valid call, and the CLI refusals of search --ranks."""
import ctypes

import numpy as np
import pytest

from tests import rank_ref

INVAL, NODEVICE, RANGE = -1, -5, -8
N_DOCS, N_TERMS, TILE = 4100, 6, 4096   # two tiles, so a doc-range shard holds less than the whole index


@pytest.fixture(scope="module")
def m(built):
    import mllm_sparse_retrieval_amd as m

    return m


@pytest.fixture(scope="module")
def idx_path(m, tmp_path_factory):
    D = np.zeros((N_DOCS, N_TERMS), dtype=np.int64)
    D[:, 0] = 1
    D[np.arange(N_DOCS), 1 + np.arange(N_DOCS) % 5] = 1 + np.arange(N_DOCS) % 9
    path = tmp_path_factory.mktemp("rank_host") / "i.idx"
    m.build_index_from_csr(str(path), *rank_ref.docs_to_csr(D), N_TERMS, doc_ids=rank_ref.doc_ids(N_DOCS), tile_docs=TILE)
    return str(path)


def call(ix, qp, qt, qw, nq, tp, to, self_ord, out=True, flags=1):
    from mllm_sparse_retrieval_amd import _cabi

    n = 0 if to is None else len(to)
    ranks, scores = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
    p = _cabi.ptr
    return _cabi.lib().msr_rank_docs(ix._h if ix is not None else None, p(qp), p(qt), p(qw), nq, flags, p(tp), p(to),
                                     p(self_ord), p(ranks) if out else None, p(scores) if out is True else None, None)


QP, QT, QW = np.array([0, 1, 2], np.int64), np.array([1, 2], np.int32), np.array([3, 4], np.int32)
TP, TO = np.array([0, 1, 3], np.int64), np.array([5, 7, 4099], np.uint32)


def test_symbol_is_exported_and_bound(m):
    from mllm_sparse_retrieval_amd import _cabi

    assert hasattr(ctypes.CDLL(_cabi.LIB_PATH), "msr_rank_docs")
    assert "msr_rank_docs" in {name for name, _, _ in _cabi.SYMBOLS}
    assert _cabi.MSR_RANK_MAX_TARGETS == 64
    header = open(m.__file__.replace("mllm_sparse_retrieval_amd/__init__.py", "include/msr.h")).read()
    assert "#define MSR_RANK_MAX_TARGETS 64" in header


def test_argument_refusals_need_no_device(m, idx_path):
    i32 = lambda *v: np.array(v, np.int32)  # noqa: E731
    with m.SparseIndex(idx_path, device=-1) as ix:
        assert call(None, QP, QT, QW, 2, TP, TO, None) == INVAL                       # null ix
        assert call(ix, None, QT, QW, 2, TP, TO, None) == INVAL                       # null q_ptr
        assert call(ix, QP, QT, QW, 2, None, TO, None) == INVAL                       # null t_ptr
        assert call(ix, QP, QT, QW, 2, TP, TO, None, out=False) == INVAL              # null out_rank
        assert call(ix, QP, QT, QW, 2, TP, TO, None, out="rank only") == INVAL        # null out_score_u32
        assert call(ix, QP, QT, QW, -1, TP, TO, None) == INVAL                        # nq < 0
        assert call(ix, QP, QT, QW, 2, np.array([1, 2, 3], np.int64), TO, None) == INVAL   # t_ptr does not start at 0
        assert call(ix, QP, QT, QW, 2, np.array([0, 2, 1], np.int64), TO, None) == INVAL   # t_ptr decreases
        assert call(ix, QP, QT, QW, 2, TP, np.array([5, 7, N_DOCS], np.uint32), None) == RANGE    # ordinal >= n_docs
        assert call(ix, QP, QT, QW, 2, TP, TO, i32(-1, N_DOCS)) == RANGE              # self_ord entry >= n_docs
        many = np.arange(m._cabi.MSR_RANK_MAX_TARGETS + 1, dtype=np.uint32)
        assert call(ix, QP, QT, QW, 2, np.array([0, 0, len(many)], np.int64), many, None) == RANGE
        assert b"MSR_RANK_MAX_TARGETS" in m._cabi.lib().msr_last_error()
        # valid calls: exactly the limit, self_ord with -1 and a real ordinal -> only the device is missing
        full = many[:-1]
        assert call(ix, QP, QT, QW, 2, np.array([0, 0, len(full)], np.int64), full, None) == NODEVICE
        assert call(ix, QP, QT, QW, 2, TP, TO, i32(-1, N_DOCS - 1)) == NODEVICE


def test_shard_handles_are_refused_before_the_device(m, idx_path):
    with m.SparseIndex(idx_path, device=-1, shard=1, n_shards=2) as sh:
        assert sh.shard_ntiles == 1 and call(sh, QP, QT, QW, 2, TP, TO, None) == INVAL
        assert b"doc-range" in m._cabi.lib().msr_last_error()
    with m.SparseIndex(idx_path, device=-1, term_shard=(0, 2)) as sh:
        assert call(sh, QP, QT, QW, 2, TP, TO, None) == INVAL
        assert b"term-range" in m._cabi.lib().msr_last_error()


def test_valid_call_without_a_device_raises(m, idx_path):
    from mllm_sparse_retrieval_amd._cabi import NoDeviceError

    with m.SparseIndex(idx_path, device=-1) as ix:
        with pytest.raises(NoDeviceError):
            ix.rank_docs(QP, QT, QW, TP, TO)
        with pytest.raises(NoDeviceError):
            ix.rank_docs(QP, QT, QW, TP, TO, self_ord=[-1, 3], drop_df_eq_n=False)
        with pytest.raises(ValueError):
            ix.rank_docs(QP, QT, QW, TP[:-1], TO)
        with pytest.raises(ValueError):
            ix.rank_docs(QP, QT, QW, TP, TO, self_ord=[1])


@pytest.mark.parametrize("argv, word", [
    (["search", "--sparse_index", "nowhere", "--passage_reps", "nowhere", "--qrels", "q.csv", "--ranks"], "--passage_reps"),
    (["search", "--sparse_index", "nowhere", "--ranks"], "--qrels"),
])
def test_cli_refuses_ranks_out_of_scope(m, argv, word):
    from mllm_sparse_retrieval_amd import cli

    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert isinstance(e.value.code, str) and "--ranks" in e.value.code and word in e.value.code   # a message = exit status 1


def test_cli_refuses_ranks_under_a_launcher(m, monkeypatch):
    from mllm_sparse_retrieval_amd import cli

    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        cli.main(["search", "--sparse_index", "nowhere", "--qrels", "q.csv", "--ranks"])
    assert isinstance(e.value.code, str) and "WORLD_SIZE" in e.value.code
