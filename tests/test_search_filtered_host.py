"""msr_search_filtered without a GPU: the symbols and MSR_FILTER_MAX_SETS, every argument refusal in its stated order
(they come before the device is looked at), the no-device refusal of a valid call, the Python layer's own checks, the
doc-set helpers of mllm_sparse_retrieval_amd.filters (packing, TSV readers) and the CLI checks of search --doc_sets."""
import ctypes

import numpy as np
import pytest

from tests import filter_ref as fr
from tests import rank_ref

INVAL, NODEVICE, RANGE = -1, -5, -8
N_DOCS, N_TERMS, TILE = 4100, 6, 4096   # two tiles, so a doc-range shard holds less than the whole index
W = (N_DOCS + 31) // 32


@pytest.fixture(scope="module")
def m(built):
    import mllm_sparse_retrieval_amd as m

    return m


@pytest.fixture(scope="module")
def idx_path(m, tmp_path_factory):
    D = np.zeros((N_DOCS, N_TERMS), dtype=np.int64)
    D[:, 0] = 1
    D[np.arange(N_DOCS), 1 + np.arange(N_DOCS) % 5] = 1 + np.arange(N_DOCS) % 9
    path = tmp_path_factory.mktemp("filtered_host") / "i.idx"
    m.build_index_from_csr(str(path), *rank_ref.docs_to_csr(D), N_TERMS, doc_ids=rank_ref.doc_ids(N_DOCS), tile_docs=TILE)
    return str(path)


QP, QT, QW = np.array([0, 1, 2], np.int64), np.array([1, 2], np.int32), np.array([3, 4], np.int32)
BITS = np.full((3, W), 0xFFFFFFFF, np.uint32)
QSET = np.array([2, -1], np.int32)


def call(ix, qp, nq, k, n_sets=3, bits=BITS, q_set=QSET, null=()):
    from mllm_sparse_retrieval_amd import _cabi

    kk = max(min(k, 2000), 1)
    o, f, u, n = np.zeros((2, kk), np.uint32), np.zeros((2, kk), np.float32), np.zeros((2, kk), np.uint32), np.zeros(2, np.int32)
    p = lambda name, a: None if name in null else _cabi.ptr(a)  # noqa: E731
    return _cabi.lib().msr_search_filtered(ix._h if ix is not None else None, _cabi.ptr(qp), _cabi.ptr(QT), _cabi.ptr(QW), nq, k,
                                           1, _cabi.ptr(bits), n_sets, _cabi.ptr(q_set), p("ord", o), p("f32", f), p("u32", u),
                                           p("n", n), None)


def test_symbols_are_exported_and_bound(m):
    from mllm_sparse_retrieval_amd import _cabi, filters

    lib = ctypes.CDLL(_cabi.LIB_PATH)
    bound = {name for name, _, _ in _cabi.SYMBOLS}
    for name in ("msr_search_filtered", "msr_dense_search_filtered"):
        assert hasattr(lib, name) and name in bound
    assert _cabi.MSR_FILTER_MAX_SETS == filters.MSR_FILTER_MAX_SETS == 65536
    header = open(m.__file__.replace("mllm_sparse_retrieval_amd/__init__.py", "include/msr.h")).read()
    assert "#define MSR_FILTER_MAX_SETS 65536" in header
    blob = open(_cabi.LIB_PATH, "rb").read()                    # the two kernels are in the gfx950 code object
    assert b"score_tiles_filtered" in blob and b"select_tiles_filtered" in blob


def test_argument_refusals_in_their_order(m, idx_path):
    err = m._cabi.lib().msr_last_error
    with m.SparseIndex(idx_path, device=-1) as ix:
        # 1. MSR_E_INVAL
        assert call(None, QP, 2, 10) == INVAL                                   # null ix
        assert call(ix, None, 2, 10) == INVAL                                   # null q_ptr
        assert call(ix, QP, -1, 10) == INVAL                                    # nq < 0
        for name in ("ord", "f32", "n"):
            assert call(ix, QP, 2, 10, null=(name,)) == INVAL                   # required outputs (out_score_u32 may be null)
        assert call(ix, QP, 2, 10, n_sets=-1) == INVAL and b"n_sets" in err()
        assert call(ix, QP, 2, 10, bits=None) == INVAL and b"set_bits" in err()  # null set_bits with n_sets > 0
        assert call(ix, QP, 2, 10, q_set=None) == INVAL and b"q_set" in err()    # null q_set with n_sets > 1
        # ... each reported before any MSR_E_RANGE cause
        bad_qset = np.array([3, 0], np.int32)
        assert call(ix, None, 2, 0) == INVAL
        assert call(ix, QP, 2, 0, bits=None) == INVAL
        assert call(ix, QP, 2, 5000, n_sets=70000, q_set=None) == INVAL
        assert call(ix, QP, 2, 10, n_sets=-1, q_set=bad_qset) == INVAL
        # 2. MSR_E_RANGE: k, then the number of sets, then the q_set entries
        for k in (0, -3, m._cabi.MSR_KMAX + 1):
            assert call(ix, QP, 2, k) == RANGE and b"MSR_KMAX" in err()
            assert call(ix, QP, 2, k, n_sets=70000) == RANGE and b"MSR_KMAX" in err()
            assert call(ix, QP, 2, k, q_set=bad_qset) == RANGE and b"MSR_KMAX" in err()
        assert call(ix, QP, 2, 10, n_sets=65537) == RANGE and b"MSR_FILTER_MAX_SETS" in err()
        assert call(ix, QP, 2, 10, n_sets=65537, q_set=np.array([70000, 0], np.int32)) == RANGE and b"MSR_FILTER_MAX_SETS" in err()
        for qs in ([3, 0], [0, -2], [-1, 3]):
            assert call(ix, QP, 2, 10, q_set=np.array(qs, np.int32)) == RANGE and b"q_set[" in err()
        assert call(ix, QP, 2, 10, n_sets=0, bits=None, q_set=np.array([0, -1], np.int32)) == RANGE   # no set to name
        # 3. valid calls: only the device is missing
        for k in (1, 10, 1024):
            assert call(ix, QP, 2, k) == NODEVICE
            assert call(ix, QP, 2, k, null=("u32",)) == NODEVICE
        assert call(ix, QP, 2, 10, n_sets=65536, q_set=np.array([65535, -1], np.int32)) == NODEVICE   # (rows are not read)
        assert call(ix, QP, 2, 10, n_sets=0, bits=None, q_set=None) == NODEVICE                   # nothing filtered
        assert call(ix, QP, 2, 10, n_sets=0, bits=None, q_set=np.array([-1, -1], np.int32)) == NODEVICE
        assert call(ix, QP, 2, 10, n_sets=1, q_set=None) == NODEVICE                              # every query uses set 0
        assert call(ix, QP, 0, 10) == NODEVICE                                                    # ... also for an empty batch


def test_shard_handles_are_refused_before_the_ranges_and_the_device(m, idx_path):
    err = m._cabi.lib().msr_last_error
    with m.SparseIndex(idx_path, device=-1, shard=1, n_shards=2) as sh:
        assert sh.shard_ntiles == 1 and call(sh, QP, 2, 10) == INVAL and b"doc-range" in err()
        assert call(sh, QP, 2, 0) == INVAL and b"doc-range" in err()
    with m.SparseIndex(idx_path, device=-1, term_shard=(0, 2)) as sh:
        assert call(sh, QP, 2, 10) == INVAL and b"term-range" in err()


def test_python_methods_without_a_device(m, idx_path):
    from mllm_sparse_retrieval_amd._cabi import MsrError, NoDeviceError

    member = np.ones((2, N_DOCS), dtype=bool)
    with m.SparseIndex(idx_path, device=-1) as ix:
        for sets in (member, fr.pack(member)):                             # bool matrix or packed words
            with pytest.raises(NoDeviceError):
                ix.search_filtered(QP, QT, QW, 10, sets, [0, -1])
        with pytest.raises(NoDeviceError):
            ix.search_filtered(QP, QT, QW, 10, member[:1])                 # one set: q_set may be left out
        with pytest.raises(NoDeviceError):
            ix.search_filtered(QP, QT, QW, 10, member[:0])                 # no set: nothing filtered
        with pytest.raises(MsrError) as e:
            ix.search_filtered(QP, QT, QW, m._cabi.MSR_KMAX + 1, member, [0, 1])
        assert e.value.code == RANGE
        with pytest.raises(MsrError) as e:
            ix.search_filtered(QP, QT, QW, 10, member, [0, 2])
        assert e.value.code == RANGE
        with pytest.raises(ValueError):
            ix.search_filtered(QP, QT, QW, 10, member)                     # two sets need q_set
        with pytest.raises(ValueError):
            ix.search_filtered(QP, QT, QW, 10, member, [0])                # one entry per query
        with pytest.raises(ValueError):
            ix.search_filtered(QP, QT, QW, 10, member[:, :-1], [0, 1])     # a matrix over another doc count
        with pytest.raises(ValueError):
            ix.search_filtered(QP, QT, QW, 10, fr.pack(member)[:, :-1], [0, 1])
        with pytest.raises(ValueError):
            ix.search_filtered(QP, QT, QW, 10, member.astype(np.int64), [0, 1])
        with pytest.raises(ValueError):
            ix.search_filtered(QP[:-1], QT, QW, 10, member, [0, 1])


def test_pack_doc_sets_and_sets_from_ordinals(m):
    from mllm_sparse_retrieval_amd import filters

    member = np.zeros((2, 70), dtype=bool)
    member[0, [0, 31, 32, 69]] = True
    member[1, 33] = True
    w = filters.pack_doc_sets(member)
    assert w.dtype == np.uint32 and w.flags.c_contiguous and w.tolist() == [[0x80000001, 1, 1 << 5], [0, 2, 0]]
    assert filters.pack_doc_sets(member[0]).tolist() == [w[0].tolist()]     # one row = one set
    assert (filters.pack_doc_sets(member.astype(np.uint8)) == w).all()
    assert (filters.sets_from_ordinals([[69, 0, 31, 32, 0], [33]], 70) == w).all()   # any order, duplicates fine
    assert filters.sets_from_ordinals([[], []], 70).tolist() == [[0, 0, 0]] * 2
    assert filters.sets_from_ordinals([], 70).shape == (0, 3)
    for bad in ([[70]], [[-1]]):
        with pytest.raises(ValueError):
            filters.sets_from_ordinals(bad, 70)
    with pytest.raises(ValueError):
        filters.pack_doc_sets(np.zeros((2, 3, 4), bool))
    member, words = fr.named_sets(2 * 4096 + 37, 4096)
    assert (filters.pack_doc_sets(member) == fr.pack(member)).all()
    assert (filters.unpack_doc_sets(words, member.shape[1]) == member).all()         # garbage above n is dropped


def test_tsv_readers(m, tmp_path):
    from mllm_sparse_retrieval_amd import filters

    d = tmp_path / "doc_sets.tsv"
    d.write_text("d1\tfold0\nd2\tfold1\n\nd3\tfold0\nd1\tfold1\n")
    assert filters.read_doc_sets(str(d)) == {"fold0": ["d1", "d3"], "fold1": ["d2", "d1"]}
    q = tmp_path / "query_sets.tsv"
    q.write_text("q1\tfold0\r\nq2\tfold1\nq1\tfold0\n")
    assert filters.read_query_sets(str(q)) == {"q1": "fold0", "q2": "fold1"}
    for text in ("d1 fold0\n", "d1\tfold0\textra\n", "\tfold0\n", "d1\t\n"):
        d.write_text(text)
        with pytest.raises(ValueError) as e:
            filters.read_doc_sets(str(d))
        assert "doc_sets.tsv:1" in str(e.value)
    q.write_text("q1\tfold0\nq1\tfold1\n")
    with pytest.raises(ValueError) as e:
        filters.read_query_sets(str(q))
    assert "q1" in str(e.value)


@pytest.mark.parametrize("argv, words", [
    (["search", "--sparse_index", "nowhere", "--doc_sets", "d.tsv"], ["--doc_sets", "--query_sets", "both"]),
    (["search", "--sparse_index", "nowhere", "--query_sets", "q.tsv"], ["--doc_sets", "--query_sets", "both"]),
    (["search", "--sparse_index", "nowhere", "--doc_sets", "d.tsv", "--query_sets", "q.tsv", "--deep", "--depth", "2000"],
     ["--doc_sets", "--deep", "--ranks", "--explain"]),
    (["search", "--sparse_index", "nowhere", "--doc_sets", "d.tsv", "--query_sets", "q.tsv", "--ranks", "--qrels", "x.csv"],
     ["--doc_sets", "--ranks"]),
    (["search", "--sparse_index", "nowhere", "--doc_sets", "d.tsv", "--query_sets", "q.tsv", "--explain", "3"],
     ["--doc_sets", "--explain"]),
    (["search", "--sparse_index", "nowhere", "--passage_reps", "nowhere", "--doc_sets", "d.tsv", "--query_sets", "q.tsv"],
     ["filtered hybrid", "--host_fusion"]),
    (["search", "--sparse_index", "nowhere", "--passage_reps", "nowhere", "--doc_sets", "d.tsv", "--query_sets", "q.tsv",
      "--fusion_union"], ["filtered hybrid", "--host_fusion"]),
    (["search", "--sparse_index", "nowhere", "--doc_sets", "d.tsv", "--query_sets", "q.tsv", "--depth", "1025"],
     ["filtered search", "MSR_KMAX = 1024", "1025"]),
    (["search", "--passage_reps", "nowhere", "--doc_sets", "d.tsv", "--query_sets", "q.tsv", "--depth", "0"],
     ["MSR_KMAX = 1024"]),
])
def test_cli_argument_checks(m, argv, words):
    from mllm_sparse_retrieval_amd import cli

    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert isinstance(e.value.code, str), e.value.code       # a message = exit status 1
    for w in words:
        assert w in e.value.code


def test_cli_help_names_the_filtered_route(m, capsys):
    from mllm_sparse_retrieval_amd import cli

    with pytest.raises(SystemExit) as e:
        cli.main(["search", "--help"])
    assert e.value.code == 0
    text = " ".join(capsys.readouterr().out.split())
    assert "--doc_sets" in text and "--query_sets" in text and "msr_search_filtered" in text
