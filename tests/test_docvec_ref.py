"""The yardstick's own check (CPU): the streamed decoder of tests/docvec_ref.py (vec range + upper bound on seg_ptr, dense
head merged) agrees with helpers.index_file_to_dense, the per-segment decoder the other suites rely on, on the golden
corpus and on a three-tile random corpus with a dense head; and the row helpers agree with each other."""
import os
import shutil

import numpy as np
import pytest

from tests import docvec_ref as dr
from tests import helpers
from tests import rank_ref as rr

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sparse_small")


@pytest.fixture(scope="module")
def m(built):
    import mllm_sparse_retrieval_amd as m

    return m


def same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and (x == y).all() for x, y in zip(a, b))


def test_decoder_on_the_golden_corpus(m, tmp_path):
    work = str(tmp_path / "enc")
    shutil.copytree(GOLD, work)
    f = helpers.read_index_file(m.build_index_from_jsonl(work))
    D = helpers.index_file_to_dense(f)
    assert D.any() and same(dr.decode_index_file(f), dr.matrix_csr(D))


def test_decoder_on_three_ragged_tiles(m, tmp_path):
    D = rr.random_corpus(2 * 4096 + 37, 300, 24, seed=1)
    path = m.build_index_from_csr(str(tmp_path / "c.idx"), *rr.docs_to_csr(D), 300, doc_ids=rr.doc_ids(len(D)), tile_docs=4096)
    f = helpers.read_index_file(path)
    assert f["n_tiles"] == 3 and (f["dense_terms"] != dr.NO_TERM).sum() >= 2
    got = dr.decode_index_file(f)
    assert same(got, dr.matrix_csr(helpers.index_file_to_dense(f))) and same(got, dr.matrix_csr(D))


def test_row_helpers():
    D = np.array([[0, 3, 0, 9], [0, 0, 0, 0], [7, 0, 65535, 0]], dtype=np.int64)
    ords = [2, 1, 2, 0]
    ptr, term, w = dr.rows_of_matrix(D, ords)
    assert ptr.tolist() == [0, 2, 2, 4, 6] and term.tolist() == [0, 2, 0, 2, 1, 3] and w.tolist() == [7, 65535, 7, 65535, 3, 9]
    assert same((ptr, term, w), dr.rows_of_csr(*rr.docs_to_csr(D), ords))
    assert same(dr.rows_of_matrix(D, []), (np.zeros(1, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.uint32)))
