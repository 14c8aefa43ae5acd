"""msr_doc_vectors without a GPU: the symbol, every argument refusal in its documented order (all of them come before the
device is looked at), shard handles, and the no-device refusal last: of a valid call, of the sizing call and of an empty
list (the n == 0 result, MSR_OK with out_ptr[0] = 0 and no launch, needs a device handle: tests/test_doc_vectors.py)."""
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
    path = tmp_path_factory.mktemp("docvec_host") / "i.idx"
    m.build_index_from_csr(str(path), *rank_ref.docs_to_csr(D), N_TERMS, doc_ids=rank_ref.doc_ids(N_DOCS), tile_docs=TILE)
    return str(path)


TO = np.array([5, 7, 4099, 5], np.uint32)


def call(ix, to, n, cap=0, out_ptr=True, arrays=False, need=True):
    from mllm_sparse_retrieval_amd import _cabi

    p = _cabi.ptr
    op, term, w = np.full(64, -1, np.int64), np.zeros(4096, np.uint32), np.zeros(4096, np.uint32)
    ne = ctypes.c_int64(-1)
    rc = _cabi.lib().msr_doc_vectors(ix._h if ix is not None else None, p(to), n, p(op) if out_ptr else None,
                                     p(term) if arrays else None, p(w) if arrays else None, cap,
                                     ctypes.byref(ne) if need else None, None)
    return rc


def test_symbol_is_exported_and_bound(m):
    from mllm_sparse_retrieval_amd import _cabi

    assert hasattr(ctypes.CDLL(_cabi.LIB_PATH), "msr_doc_vectors")
    assert "msr_doc_vectors" in {name for name, _, _ in _cabi.SYMBOLS}
    header = open(m.__file__.replace("mllm_sparse_retrieval_amd/__init__.py", "include/msr.h")).read()
    assert "int msr_doc_vectors(" in header


def test_argument_refusals_need_no_device(m, idx_path):
    err = lambda: m._cabi.lib().msr_last_error()  # noqa: E731
    with m.SparseIndex(idx_path, device=-1) as ix:
        assert call(None, TO, 4) == INVAL                                   # null ix
        assert call(ix, TO, 4, out_ptr=False) == INVAL                      # null out_ptr
        assert call(ix, TO, 4, need=False) == INVAL                         # null n_entries
        assert call(ix, None, 4) == INVAL                                   # null t_ord with n > 0
        assert b"t_ord" in err()
        assert call(ix, TO, -1) == INVAL                                    # n < 0
        assert call(ix, TO, 4, cap=-1) == INVAL                             # cap < 0
        assert call(ix, TO, 4, cap=1) == INVAL                              # null out_term / out_w with cap > 0
        assert b"cap" in err()
        # order: the shapes (INVAL) are reported before a bad ordinal (RANGE) ...
        bad = np.array([5, N_DOCS, 7], np.uint32)
        assert call(ix, bad, 3, cap=-1) == INVAL
        assert call(ix, bad, 3, cap=1) == INVAL
        assert call(ix, bad, 3) == RANGE                                    # ordinal >= n_docs
        assert b"outside the index" in err()
        assert call(ix, bad, 3, cap=4096, arrays=True) == RANGE
        assert call(ix, bad, 1) == NODEVICE                                 # (only the listed entries are looked at)
        # ... and the device comes last: valid calls miss only the device
        assert call(ix, TO, 4) == NODEVICE                                  # the sizing call
        assert call(ix, TO, 4, cap=4096, arrays=True) == NODEVICE
        assert call(ix, np.arange(N_DOCS, dtype=np.uint32), N_DOCS) == NODEVICE     # every doc of the index
        assert call(ix, None, 0) == NODEVICE                                # an empty list: still no device
        assert b"no HIP device" in err()


def test_shard_handles_are_refused_before_the_device(m, idx_path):
    with m.SparseIndex(idx_path, device=-1, shard=1, n_shards=2) as sh:
        assert sh.shard_ntiles == 1 and call(sh, TO, 4) == INVAL
        assert b"doc-range" in m._cabi.lib().msr_last_error()
        assert call(sh, np.array([N_DOCS], np.uint32), 1) == RANGE          # a bad ordinal comes before the handle's kind
    with m.SparseIndex(idx_path, device=-1, term_shard=(0, 2)) as sh:
        assert call(sh, TO, 4) == INVAL
        assert b"term-range" in m._cabi.lib().msr_last_error()


def test_valid_call_without_a_device_raises(m, idx_path):
    from mllm_sparse_retrieval_amd._cabi import NoDeviceError

    with m.SparseIndex(idx_path, device=-1) as ix:
        with pytest.raises(NoDeviceError):
            ix.doc_vectors(TO)
        with pytest.raises(NoDeviceError):
            ix.doc_vectors(TO, with_ms=True)
        with pytest.raises(ValueError):
            ix.doc_vectors(TO.reshape(2, 2))


def test_search_docs_depth_limit_needs_no_index(m):
    from mllm_sparse_retrieval_amd import searcher

    s = searcher.LuceneImpactSearcher.__new__(searcher.LuceneImpactSearcher)   # the check comes before the index is touched
    with pytest.raises(ValueError):
        s.batch_search_docs(["x"], k=m._cabi.MSR_KMAX, remove_self=True)
    with pytest.raises(ValueError):
        s.batch_search_docs(["x"], k=0)
