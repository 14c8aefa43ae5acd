"""msr_dense_search_filtered without a GPU: what can be reached without a dense handle (one cannot be opened without a
device): the null-handle / null-output refusal and its place before every other cause, and the Python layer's checks of
doc sets and q_set, which run before the C call. The refusals that need a handle (precision mismatch, k, the sets' ranges,
in their order) are checked on the GPU: tests/test_dense_filtered.py::test_refusals_in_their_order."""
import numpy as np
import pytest

INVAL = -1


@pytest.fixture(scope="module")
def m(built):
    import mllm_sparse_retrieval_amd as m

    return m


def test_null_handle_is_refused_first(m):
    from mllm_sparse_retrieval_amd import _cabi

    lib, p = _cabi.lib(), _cabi.ptr
    q = np.zeros((1, 4), np.float32)
    out, n = np.zeros(8, np.uint32), np.zeros(1, np.int32)
    bits, qs = np.ones((2, 1), np.uint32), np.array([5], np.int32)
    # null dx, together with a bad k, too many sets and a q_set entry out of range: MSR_E_INVAL wins
    for k, n_sets in ((8, 2), (0, 2), (8, 70000), (5000, -1)):
        rc = lib.msr_dense_search_filtered(None, p(q), 1, 1, k, p(bits), n_sets, p(qs), p(out), p(out), p(n), None)
        assert rc == INVAL and b"msr_dense_search_filtered" in lib.msr_last_error()
    from mllm_sparse_retrieval_amd.dense import DenseIndex

    with pytest.raises(_cabi.NoDeviceError):
        DenseIndex(np.zeros((4, 32), np.float32), device=-1)


def test_python_checks_of_sets_and_q_set(m):
    from mllm_sparse_retrieval_amd import filters

    n = 70
    member = np.zeros((2, n), dtype=bool)
    member[0, ::2] = True
    packed = filters.as_packed_sets(member, n)
    assert packed.dtype == np.uint32 and packed.shape == (2, 3) and (packed == filters.pack_doc_sets(member)).all()
    assert filters.as_packed_sets(packed, n) is not None and (filters.as_packed_sets(packed, n) == packed).all()
    assert filters.as_packed_sets(member[0], n).shape == (1, 3) and filters.as_packed_sets(packed[0], n).shape == (1, 3)
    assert filters.as_packed_sets(member[:0], n).shape == (0, 3)
    for bad in (member[:, :-1], packed[:, :-1], member.astype(np.float32), np.zeros((2, 2, 2), bool)):
        with pytest.raises(ValueError):
            filters.as_packed_sets(bad, n)
    assert filters.as_q_set(None, 4, 0) is None and filters.as_q_set(None, 4, 1) is None
    with pytest.raises(ValueError):
        filters.as_q_set(None, 4, 2)
    qs = filters.as_q_set([0, -1, 1, 0], 4, 2)
    assert qs.dtype == np.int32 and qs.tolist() == [0, -1, 1, 0]
    with pytest.raises(ValueError):
        filters.as_q_set([0, 1], 4, 2)


def test_searcher_classes_have_the_filtered_methods(m):
    from mllm_sparse_retrieval_amd.dense import DenseIndex, FaissFlatSearcher
    from mllm_sparse_retrieval_amd.searcher import LuceneImpactSearcher

    for cls, name in ((DenseIndex, "search_filtered"), (DenseIndex, "search_keys_filtered"), (FaissFlatSearcher, "search_filtered"),
                      (LuceneImpactSearcher, "batch_search_filtered"), (m.SparseIndex, "search_filtered")):
        assert callable(getattr(cls, name))
