"""f32 flat dense search on the GPU (msr_dense_search_f32, DenseIndex(precision="f32"), dense-only `search`): keys
bit-equal to the k-ordered fmaf chain (tests/f32_chain.py), ties to the lower row, batch invariance, accuracy
against float64, the scratch kept on the handle, misuse refused, and the search_dense.sh recipe end to end."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.f32_chain import chain_scores, f32_keys, topk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def m(built):
    import mllm_sparse_retrieval_amd as m

    return m


def _rows(rng, n, h, dup_every=0):
    x = rng.standard_normal((n, h)).astype(np.float32)
    if dup_every and n > dup_every:
        x[dup_every::dup_every] = x[0]  # bit-equal rows: score ties the lower row must win
    return x


def _check(dix, q, want_scores, k):
    idx, key, n = dix.search_keys(q, k)
    w_idx, w_key, w_n = topk(want_scores, k)
    assert (n == w_n).all()
    bad = np.argwhere(key != w_key)
    assert bad.size == 0, f"k={k}: {len(bad)} keys differ, first at {bad[0]}: {key[tuple(bad[0])]:#x} vs {w_key[tuple(bad[0])]:#x}"
    assert (idx == w_idx).all(), f"k={k}: ids differ at {np.argwhere(idx != w_idx)[0]}"


@pytest.mark.parametrize("h", [1, 3, 31, 100, 256])
@pytest.mark.parametrize("n_docs", [3, 700, 9000])
def test_bitwise_fmaf_chain(m, h, n_docs):
    from mllm_sparse_retrieval_amd.dense import DenseIndex

    rng = np.random.default_rng(h * 1000 + n_docs)
    p = _rows(rng, n_docs, h, dup_every=97)
    q = _rows(rng, 300, h)
    want = chain_scores(q, p)
    dix = DenseIndex(p, device=0, precision="f32")
    try:
        assert dix.precision == "f32"
        for nq in (1, 130, 300):
            for k in (1, 10, 1000):
                _check(dix, q[:nq], want[:nq], k)
    finally:
        dix.close()


def test_bitwise_sampled_h4096(m):
    from mllm_sparse_retrieval_amd.dense import DenseIndex

    rng = np.random.default_rng(4096)
    p = _rows(rng, 9000, 4096, dup_every=1000)
    q = _rows(rng, 300, 4096)
    dix = DenseIndex(p, device=0, precision="f32")
    try:
        idx, key, n = dix.search_keys(q, 100)
    finally:
        dix.close()
    sample = np.array([0, 1, 137, 256, 299])
    w_idx, w_key, w_n = topk(chain_scores(q[sample], p), 100)
    assert (key[sample] == w_key).all() and (idx[sample] == w_idx).all() and (n == 100).all()


def test_against_float64_and_fp16(m):
    from mllm_sparse_retrieval_amd.dense import DenseIndex

    rng = np.random.default_rng(7)
    h, n, nq = 4096, 25010, 500
    p = rng.standard_normal((n, h)).astype(np.float32)
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    q = (p[rng.integers(0, n, nq)] + 0.05 * rng.standard_normal((nq, h))).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    errs = {}
    for prec in ("f32", "fp16"):
        dix = DenseIndex(p, device=0, precision=prec)
        try:
            s, i = dix.search(q, 10)
        finally:
            dix.close()
        s64 = np.einsum("qh,qkh->qk", q.astype(np.float64), p[i].astype(np.float64))
        errs[prec] = float(np.abs(s - s64).max())
    assert errs["f32"] <= 2e-6, errs
    assert errs["f32"] * 10 <= errs["fp16"], errs


def test_near_duplicates_below_fp16_resolution(m):
    from mllm_sparse_retrieval_amd.dense import DenseIndex

    rng = np.random.default_rng(11)
    h = 256
    b = (rng.uniform(2.0 ** -6, 1.0, h) * rng.choice([-1.0, 1.0], h)).astype(np.float16).astype(np.float32)
    steps = np.array([5, 2, 7, 0, 3, 6, 1, 4])  # row r holds b * (1 + steps[r] * 2^-16): one fp16 row for all
    p = (b[None, :] * (1 + steps[:, None] * 2.0 ** -16)).astype(np.float32)
    assert (p.astype(np.float16) == b.astype(np.float16)).all()
    q = (b / np.linalg.norm(b))[None, :].astype(np.float32)
    want = np.argsort(-steps, kind="stable")
    d32 = DenseIndex(p, device=0, precision="f32")
    d16 = DenseIndex(p, device=0, precision="fp16")
    try:
        idx, key, _ = d32.search_keys(q, 8)
        assert idx[0].tolist() == want.tolist()
        assert len(set(key[0].tolist())) == 8
        w_idx, w_key, _ = topk(chain_scores(q, p), 8)
        assert (idx == w_idx).all() and (key == w_key).all()
        idx16, key16, _ = d16.search_keys(q, 8)
        assert len(set(key16[0].tolist())) == 1 and idx16[0].tolist() == list(range(8))  # fp16: one tie, row order
    finally:
        d32.close()
        d16.close()


def test_batch_invariance(m):
    from mllm_sparse_retrieval_amd.dense import FaissFlatSearcher

    rng = np.random.default_rng(3)
    p = _rows(rng, 9000, 100, dup_every=50)
    q = _rows(rng, 300, 100)
    fs = FaissFlatSearcher(p, device=0, precision="f32")
    fs.add(p)
    ref_s, ref_i = fs.search(q, 50)
    for bs in (1, 2, 97, 300):
        s, i = fs.batch_search(q, 50, bs)
        assert (s.view(np.uint32) == ref_s.view(np.uint32)).all() and (i == ref_i).all(), bs
    w_idx, w_key, _ = topk(chain_scores(q[:20], p), 50)
    assert (ref_i[:20] == w_idx).all() and (f32_keys(ref_s[:20]) == w_key).all()


def test_scratch_stays_on_the_handle(m):
    from mllm_sparse_retrieval_amd.dense import DenseIndex

    rng = np.random.default_rng(4)
    p, q = _rows(rng, 5000, 64), _rows(rng, 600, 64)
    dix = DenseIndex(p, device=0, precision="f32")
    try:
        a = dix.search(q, 10)
        st = dix.stats()
        assert st["device_allocs"] > 0
        for _ in range(3):
            b = dix.search(q, 10)
            assert (a[1] == b[1]).all()
        assert dix.stats() == st
    finally:
        dix.close()


def test_misuse_and_edges(m, tmp_path):
    from mllm_sparse_retrieval_amd import _cabi
    from mllm_sparse_retrieval_amd._cabi import MsrError
    from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_search

    L = _cabi.lib()
    rng = np.random.default_rng(5)
    p, q = _rows(rng, 3, 40), _rows(rng, 4, 40)
    d32 = DenseIndex(p, device=0, precision="f32")
    d16 = DenseIndex(p, device=0)
    try:
        idx = np.zeros((4, 2), np.uint32)
        key = np.zeros((4, 2), np.uint32)
        n = np.zeros(4, np.int32)
        q16 = np.zeros((4, 64), np.float16)
        a, b = ctypes.c_float(), ctypes.c_float()
        rc = L.msr_dense_search(d32._h, _cabi.ptr(q16), 4, 2, _cabi.ptr(idx), _cabi.ptr(key), _cabi.ptr(n),
                                ctypes.byref(a), ctypes.byref(b))
        assert rc == -1 and b"msr_dense_search_f32" in L.msr_last_error()
        rc = L.msr_dense_search_f32(d16._h, _cabi.ptr(q), 4, 2, _cabi.ptr(idx), _cabi.ptr(key), _cabi.ptr(n),
                                    ctypes.byref(a), ctypes.byref(b))
        assert rc == -1 and b"msr_dense_search" in L.msr_last_error()
        for k in (0, 1025):
            with pytest.raises(MsrError) as e:
                d32.search(q, k)
            assert e.value.code == -8  # MSR_E_RANGE
        s, i = d32.search(np.zeros((0, 40), np.float32), 5)  # no queries
        assert s.shape == (0, 5) and i.shape == (0, 5)
        s, i = d32.search(q, 10)  # corpus smaller than k
        assert (i[:, 3:] == -1).all() and np.isneginf(s[:, 3:]).all() and (np.sort(i[:, :3], axis=1) == [0, 1, 2]).all()
        w_idx, w_key, _ = topk(chain_scores(q, p), 10)
        assert (i[:, :3] == w_idx[:, :3]).all() and (f32_keys(s[:, :3]) == w_key[:, :3]).all()
        # the hybrid path takes fp16 handles only: refused in Python and in the C-ABI
        dp = np.array([0, 1, 2, 3], dtype=np.uint64)
        path = m.build_index_from_csr(str(tmp_path / "i.idx"), dp, np.array([0, 1, 0], np.uint32),
                                      np.array([3, 2, 1], np.uint32), 2, tile_docs=4096)
        with m.SparseIndex(path, device=0) as ix:
            qp, qt, qw = np.array([0, 1, 2, 3, 4]), np.array([0, 1, 0, 1]), np.array([1, 1, 1, 1])
            r2o = np.arange(3, dtype=np.uint32)
            with pytest.raises(ValueError):
                hybrid_search(ix, d32, qp, qt, qw, q, 2, 2, 0.5, r2o)
            qp, qt, qw = _cabi.as_csr(qp, qt, qw)
            ords, sc = np.zeros((4, 2), np.uint32), np.zeros((4, 2), np.float32)
            ms = (ctypes.c_float * 4)()
            rc = L.msr_hybrid_search(ix._h, d32._h, _cabi.ptr(qp), _cabi.ptr(qt), _cabi.ptr(qw), _cabi.ptr(q16), 4, 2, 2,
                                     0.5, 0, _cabi.ptr(r2o), None, _cabi.ptr(ords), _cabi.ptr(sc), _cabi.ptr(n), ms)
            assert rc == -1 and b"f32" in L.msr_last_error()
    finally:
        d32.close()
        d16.close()


def _run_cli(*args, cwd):
    r = subprocess.run([sys.executable, "-m", "mllm_sparse_retrieval_amd", *args], cwd=cwd, capture_output=True,
                       text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_cli_dense_only_search(m, tmp_path):
    import pickle

    from mllm_sparse_retrieval_amd.cli import normalize_rows
    from mllm_sparse_retrieval_amd.dense import FaissFlatSearcher
    from mllm_sparse_retrieval_amd.fusion import read_trec_run
    from mllm_sparse_retrieval_amd.run import get_run_dict

    out, dense = str(tmp_path / "sp"), str(tmp_path / "dense")
    _run_cli("encode", "--synthetic", "coco", "--n_images", "400", "--sparse_output_dir", out, "--dense_output_dir",
             dense, "--dense_dim", "100", cwd=str(tmp_path))
    with open(os.path.join(dense, "corpus_0.pkl"), "rb") as f:
        p, p_lookup = pickle.load(f)
    with open(os.path.join(dense, "query.pkl"), "rb") as f:
        qv, q_lookup = pickle.load(f)
    qids = [str(x) for x in q_lookup]
    q = normalize_rows(qv)
    lookup = np.asarray([str(x) for x in p_lookup], dtype=object)

    def expect(scores, idx):
        return get_run_dict(qids, scores, lookup[idx], True)

    w_idx, w_key, _ = topk(chain_scores(q, p), 10)
    from mllm_sparse_retrieval_amd.dense import keys_to_f32

    runs = {"f32": expect(keys_to_f32(w_key), w_idx.astype(np.int64))}
    fs = FaissFlatSearcher(p, device=0)
    fs.add(p)
    runs["fp16"] = expect(*fs.search(q, 10))
    for prec, extra in (("f32", []), ("fp16", ["--use_gpu"])):
        save = str(tmp_path / f"runs_{prec}")
        text = _run_cli("search", "--passage_reps", dense, "--depth", "10", "--remove_query", "--qrels",
                        os.path.join(out, "qrels.csv"), "--query_type", "text", "--save_dir", save, *extra,
                        cwd=str(tmp_path))
        assert sorted(os.listdir(save)) == ["dense.trec"]
        assert "Dense recall @ 1" in text and "Sparse" not in text and "Fusion" not in text
        got = read_trec_run(os.path.join(save, "dense.trec"))
        want = runs[prec]
        assert list(got) == [x for x in qids if want[x]["docs"]]
        for qid in got:
            assert list(got[qid]["docs"]) == list(want[qid]["docs"]), (prec, qid)
            assert [np.float32(v) for v in got[qid]["docs"].values()] == [np.float32(v) for v in want[qid]["docs"].values()]
