"""The deep calls without a GPU: the symbols and MSR_DEEP_KMAX, every argument refusal in its order (they come before the
device is looked at), the no-device refusal of a valid call, and the CLI checks of search --deep."""
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
    path = tmp_path_factory.mktemp("deep_host") / "i.idx"
    m.build_index_from_csr(str(path), *rank_ref.docs_to_csr(D), N_TERMS, doc_ids=rank_ref.doc_ids(N_DOCS), tile_docs=TILE)
    return str(path)


QP, QT, QW = np.array([0, 1, 2], np.int64), np.array([1, 2], np.int32), np.array([3, 4], np.int32)


def call(ix, qp, nq, k, null=()):
    from mllm_sparse_retrieval_amd import _cabi

    kk = max(min(k, 20000), 1)
    o, f, u, n = np.zeros((2, kk), np.uint32), np.zeros((2, kk), np.float32), np.zeros((2, kk), np.uint32), np.zeros(2, np.int32)
    p = lambda name, a: None if name in null else _cabi.ptr(a)  # noqa: E731
    return _cabi.lib().msr_search_deep(ix._h if ix is not None else None, _cabi.ptr(qp), _cabi.ptr(QT), _cabi.ptr(QW), nq, k, 1,
                                       p("ord", o), p("f32", f), p("u32", u), p("n", n), None)


def test_symbols_are_exported_and_bound(m):
    from mllm_sparse_retrieval_amd import _cabi

    lib = ctypes.CDLL(_cabi.LIB_PATH)
    bound = {name for name, _, _ in _cabi.SYMBOLS}
    for name in ("msr_search_deep", "msr_dense_search_deep"):
        assert hasattr(lib, name) and name in bound
    assert _cabi.MSR_DEEP_KMAX == 16384 and _cabi.MSR_KMAX == 1024
    header = open(m.__file__.replace("mllm_sparse_retrieval_amd/__init__.py", "include/msr.h")).read()
    assert "#define MSR_DEEP_KMAX 16384" in header
    assert b"deep_select_rows" in open(_cabi.LIB_PATH, "rb").read()      # the kernel is in the gfx950 code object


def test_argument_refusals_in_their_order(m, idx_path):
    kmax = m._cabi.MSR_DEEP_KMAX
    err = m._cabi.lib().msr_last_error
    with m.SparseIndex(idx_path, device=-1) as ix:
        assert call(None, QP, 2, 2000) == INVAL                      # null ix
        assert call(ix, None, 2, 2000) == INVAL                      # null q_ptr
        assert call(ix, QP, -1, 2000) == INVAL                       # nq < 0
        for name in ("ord", "f32", "n"):
            assert call(ix, QP, 2, 2000, null=(name,)) == INVAL      # null outputs (out_score_u32 alone may be null)
        assert call(ix, None, 2, 0) == INVAL                         # ... reported before k
        for k in (0, -3, kmax + 1):
            assert call(ix, QP, 2, k) == RANGE and b"MSR_DEEP_KMAX" in err()
        for k in (1, 1024, 1025, kmax):                              # valid: only the device is missing
            assert call(ix, QP, 2, k) == NODEVICE
            assert call(ix, QP, 2, k, null=("u32",)) == NODEVICE
        assert call(ix, QP, 0, 2000) == NODEVICE                     # ... also for an empty batch, as the order says


def test_shard_handles_are_refused_before_the_device(m, idx_path):
    err = m._cabi.lib().msr_last_error
    with m.SparseIndex(idx_path, device=-1, shard=1, n_shards=2) as sh:
        assert sh.shard_ntiles == 1 and call(sh, QP, 2, 2000) == INVAL and b"doc-range" in err()
    with m.SparseIndex(idx_path, device=-1, term_shard=(0, 2)) as sh:
        assert call(sh, QP, 2, 2000) == INVAL and b"term-range" in err()


def test_python_methods_without_a_device(m, idx_path):
    from mllm_sparse_retrieval_amd._cabi import MsrError, NoDeviceError

    with m.SparseIndex(idx_path, device=-1) as ix:
        with pytest.raises(NoDeviceError):
            ix.search_deep(QP, QT, QW, 2000)
        with pytest.raises(MsrError) as e:
            ix.search_deep(QP, QT, QW, m._cabi.MSR_DEEP_KMAX + 1)
        assert e.value.code == RANGE
        with pytest.raises(ValueError):
            ix.search_deep(QP[:-1], QT, QW, 2000)


def test_dense_null_handle_and_outputs_are_refused(m):
    from mllm_sparse_retrieval_amd import _cabi

    q = np.zeros((1, 4), np.float32)
    out, n = np.zeros(8, np.uint32), np.zeros(1, np.int32)
    p = _cabi.ptr
    rc = _cabi.lib().msr_dense_search_deep(None, p(q), 1, 1, 8, p(out), p(out), p(n), None)
    assert rc == INVAL and b"msr_dense_search_deep" in _cabi.lib().msr_last_error()
    # (a dense handle cannot be opened without a device: the q_is_f32 mismatch and the k range of this call are checked
    # on the GPU, tests/test_dense_deep.py::test_refusals)
    from mllm_sparse_retrieval_amd.dense import DenseIndex

    with pytest.raises(_cabi.NoDeviceError):
        DenseIndex(np.zeros((4, 32), np.float32), device=-1)


@pytest.mark.parametrize("argv, words", [
    (["search", "--sparse_index", "nowhere", "--deep", "--depth", "16385"], ["MSR_DEEP_KMAX", "16385"]),
    (["search", "--passage_reps", "nowhere", "--deep", "--depth", "16385"], ["MSR_DEEP_KMAX", "16385"]),
    (["search", "--sparse_index", "nowhere", "--deep", "--depth", "0"], ["MSR_DEEP_KMAX"]),
    (["search", "--sparse_index", "nowhere", "--passage_reps", "nowhere", "--deep", "--depth", "2000"], ["--deep", "--host_fusion"]),
    (["search", "--sparse_index", "nowhere", "--passage_reps", "nowhere", "--deep", "--fusion_union", "--depth", "2000"],
     ["--deep", "--fusion_union"]),
    (["search", "--sparse_index", "nowhere", "--passage_reps", "nowhere", "--deep", "--host_fusion", "--hybrid_f32"],
     ["--deep", "--hybrid_f32"]),
    # without --deep the old messages stand
    (["search", "--passage_reps", "nowhere", "--depth", "1025"], ["MSR_KMAX = 1024", "dense-only"]),
    (["search", "--sparse_index", "nowhere", "--passage_reps", "nowhere", "--fusion_union", "--depth", "1025"],
     ["--fusion_union", "MSR_KMAX = 1024"]),
    (["search", "--sparse_index", "nowhere", "--passage_reps", "nowhere", "--fusion_union", "--host_fusion"],
     ["--fusion_union", "--host_fusion", "contradict"]),
])
def test_cli_argument_checks(m, argv, words):
    from mllm_sparse_retrieval_amd import cli

    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert isinstance(e.value.code, str), e.value.code       # a message = exit status 1
    for w in words:
        assert w in e.value.code
    assert ("--deep" in e.value.code) == ("--deep" in argv)


def test_cli_help_names_the_deep_route(m, capsys):
    from mllm_sparse_retrieval_amd import cli

    with pytest.raises(SystemExit) as e:
        cli.main(["search", "--help"])
    assert e.value.code == 0
    text = " ".join(capsys.readouterr().out.split())
    assert "--deep" in text and "MSR_DEEP_KMAX" in text and "msr_search_deep" in text
