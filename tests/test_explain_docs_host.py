"""msr_explain_docs without a GPU: the symbol, every argument refusal in its documented order (all of them come before
the device is looked at), the no-device refusal of a valid call, shard handles, explain.py's rows and TSV text on a
hand-made result, and the CLI refusals of search --explain."""
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
    path = tmp_path_factory.mktemp("explain_host") / "i.idx"
    m.build_index_from_csr(str(path), *rank_ref.docs_to_csr(D), N_TERMS, doc_ids=rank_ref.doc_ids(N_DOCS), tile_docs=TILE)
    return str(path)


QP, QT, QW = np.array([0, 1, 3], np.int64), np.array([1, 2, 3], np.int32), np.array([3, 4, 5], np.int32)
TP, TO = np.array([0, 1, 3], np.int64), np.array([5, 7, 4099], np.uint32)
NEED = 1 * 1 + 2 * 2     # one listed doc of the one-entry query, two of the two-entry query


def call(ix, qp, qt, qw, nq, tp, to, cap=None, out=True, flags=1):
    from mllm_sparse_retrieval_amd import _cabi

    buf = np.zeros(4096, np.uint32)
    p = _cabi.ptr
    return _cabi.lib().msr_explain_docs(ix._h if ix is not None else None, p(qp), p(qt), p(qw), nq, flags, p(tp), p(to),
                                        p(buf) if out else None, NEED if cap is None else cap, None)


def test_symbol_is_exported_and_bound(m):
    from mllm_sparse_retrieval_amd import _cabi

    assert hasattr(ctypes.CDLL(_cabi.LIB_PATH), "msr_explain_docs")
    assert "msr_explain_docs" in {name for name, _, _ in _cabi.SYMBOLS}
    assert _cabi.MSR_EXPLAIN_MAX_TARGETS == 64
    header = open(m.__file__.replace("mllm_sparse_retrieval_amd/__init__.py", "include/msr.h")).read()
    assert "#define MSR_EXPLAIN_MAX_TARGETS 64" in header and "int msr_explain_docs(" in header


def test_argument_refusals_need_no_device(m, idx_path):
    i64 = lambda *v: np.array(v, np.int64)  # noqa: E731
    err = lambda: m._cabi.lib().msr_last_error()  # noqa: E731
    with m.SparseIndex(idx_path, device=-1) as ix:
        assert call(None, QP, QT, QW, 2, TP, TO) == INVAL                       # null ix
        assert call(ix, None, QT, QW, 2, TP, TO) == INVAL                       # null q_ptr
        assert call(ix, QP, QT, QW, 2, None, TO) == INVAL                       # null t_ptr
        assert call(ix, QP, QT, QW, 2, TP, TO, out=False) == INVAL              # null out_doc_w
        assert call(ix, QP, QT, QW, -1, TP, TO) == INVAL                        # nq < 0
        assert call(ix, QP, QT, QW, 2, i64(1, 2, 3), TO) == INVAL               # t_ptr does not start at 0
        assert call(ix, QP, QT, QW, 2, i64(0, 2, 1), TO) == INVAL               # t_ptr decreases
        assert call(ix, QP, QT, QW, 2, TP, None) == INVAL                       # null t_ord with entries
        assert call(ix, i64(0, 2, 1), QT, QW, 2, TP, TO) == INVAL               # q_ptr decreases
        assert call(ix, QP, None, QW, 2, TP, TO) == INVAL                       # null q_term with entries
        assert call(ix, QP, QT, QW, 2, TP, TO, cap=NEED - 1) == INVAL           # out_cap one short
        assert b"out_cap" in err()
        assert call(ix, QP, QT, QW, 2, TP, TO, cap=-1) == INVAL
        # order: a short out_cap (INVAL) is reported before a bad ordinal or too many targets (RANGE) ...
        bad_ord = np.array([5, 7, N_DOCS], np.uint32)
        assert call(ix, QP, QT, QW, 2, TP, bad_ord, cap=NEED - 1) == INVAL
        assert call(ix, QP, QT, QW, 2, TP, bad_ord) == RANGE                    # ordinal >= n_docs
        many = np.arange(m._cabi.MSR_EXPLAIN_MAX_TARGETS + 1, dtype=np.uint32)
        tp_many = i64(0, 0, len(many))
        assert call(ix, QP, QT, QW, 2, tp_many, many, cap=2 * len(many) - 1) == INVAL
        assert call(ix, QP, QT, QW, 2, tp_many, many, cap=2 * len(many)) == RANGE
        assert b"MSR_EXPLAIN_MAX_TARGETS" in err()
        # ... and the device comes last: valid calls, exactly the limit included, miss only the device
        full = many[:-1]
        assert call(ix, QP, QT, QW, 2, i64(0, 0, len(full)), full, cap=2 * len(full)) == NODEVICE
        assert call(ix, QP, QT, QW, 2, TP, TO) == NODEVICE
        assert call(ix, QP, QT, QW, 2, TP, TO, cap=NEED + 100, flags=0) == NODEVICE
        assert call(ix, QP, QT, QW, 2, i64(0, 0, 0), None, cap=0) == NODEVICE   # no target at all: still no device
        # a query error the normalisation reports (term id outside the dictionary) needs the device's handle: it
        # comes after MSR_E_NODEVICE, as in msr_rank_docs
        assert call(ix, QP, np.array([1, 2, N_TERMS], np.int32), QW, 2, TP, TO) == NODEVICE


def test_shard_handles_are_refused_before_the_device(m, idx_path):
    with m.SparseIndex(idx_path, device=-1, shard=1, n_shards=2) as sh:
        assert sh.shard_ntiles == 1 and call(sh, QP, QT, QW, 2, TP, TO) == INVAL
        assert b"doc-range" in m._cabi.lib().msr_last_error()
    with m.SparseIndex(idx_path, device=-1, term_shard=(0, 2)) as sh:
        assert call(sh, QP, QT, QW, 2, TP, TO) == INVAL
        assert b"term-range" in m._cabi.lib().msr_last_error()


def test_valid_call_without_a_device_raises(m, idx_path):
    from mllm_sparse_retrieval_amd._cabi import NoDeviceError

    with m.SparseIndex(idx_path, device=-1) as ix:
        with pytest.raises(NoDeviceError):
            ix.explain_docs(QP, QT, QW, TP, TO)
        with pytest.raises(NoDeviceError):
            ix.explain_docs(QP, QT, QW, TP, TO, drop_df_eq_n=False, with_ms=True)
        with pytest.raises(ValueError):
            ix.explain_docs(QP, QT, QW, TP[:-1], TO)
        with pytest.raises(ValueError):
            ix.explain_docs(QP, QT, QW, np.array([0, 2, 1], np.int64), TO[:1])


# --------------------------------------------------------------------------------------------- explain.py on a made result
def test_rows_and_tsv_text():
    from mllm_sparse_retrieval_amd import explain as ex

    # two queries; query 0 = "cat cat dog zebra the" as CSR with a repeated token, an entry that does not count (the)
    # and one the docs lack (zebra); it lists two docs, query 1 ("b\xc3\xa9 a") lists one doc it does not match at all
    q_ptr = [0, 5, 7]
    tokens = ["cat", "dog", "zebra", "the", "cat", "bé", "a"]
    q_w = [2, 1, 4, 3, 1, 1, 1]
    t_ptr = [0, 2, 3]
    x_ptr = [0, 5, 10, 12]
    doc_w = [3, 9, 0, 0, 3,   40000, 0, 0, 0, 40000,   0, 0]
    rows = ex.build_rows(q_ptr, tokens, q_w, t_ptr, x_ptr, doc_w)
    assert rows == [[("cat", 3, 3, 9), ("dog", 1, 9, 9)],          # a tie in contribution: token bytes decide
                    [("cat", 3, 40000, 120000)],
                    []]
    assert [ex.score_of(r) for r in rows] == [18, 120000, 0]
    # equal contributions: tokens in bytewise (UTF-8) order
    assert ex.rows_of(["é", "z", "a"], [1, 1, 1], [5, 5, 5]) == [("a", 1, 5, 5), ("z", 1, 5, 5), ("é", 1, 5, 5)]
    recs = [("q0", "d7", 1, True, rows[0]), ("q0", "d9", 0, False, rows[1]), ("q1", "d7", 0, True, rows[2])]
    text = "".join(ex.tsv_lines(recs))
    assert text == ("q0\td7\t1\t1\t18\tcat\t3\t3\t9\n"
                    "q0\td7\t1\t1\t18\tdog\t1\t9\t9\n"
                    "q0\td9\t0\t0\t120000\tcat\t3\t40000\t120000\n"
                    "q1\td7\t0\t1\t0\t-\t0\t0\t0\n")
    assert len(ex.TSV_COLUMNS) == len(text.splitlines()[0].split("\t"))
    with pytest.raises(ValueError):
        ex.build_rows(q_ptr, tokens, q_w, t_ptr, [0, 5, 9, 11], doc_w)


@pytest.mark.parametrize("argv, word", [
    (["search", "--sparse_index", "nowhere", "--passage_reps", "nowhere", "--explain", "3"], "--passage_reps"),
    (["search", "--sparse_index", "nowhere", "--explain", "0"], "MSR_EXPLAIN_MAX_TARGETS"),
    (["search", "--sparse_index", "nowhere", "--explain", "65"], "MSR_EXPLAIN_MAX_TARGETS"),
])
def test_cli_refuses_explain_out_of_scope(m, argv, word):
    from mllm_sparse_retrieval_amd import cli

    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert isinstance(e.value.code, str) and "--explain" in e.value.code and word in e.value.code   # a message = exit status 1


def test_cli_refuses_explain_under_a_launcher(m, monkeypatch):
    from mllm_sparse_retrieval_amd import cli

    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        cli.main(["search", "--sparse_index", "nowhere", "--explain", "3"])
    assert isinstance(e.value.code, str) and "WORLD_SIZE" in e.value.code
