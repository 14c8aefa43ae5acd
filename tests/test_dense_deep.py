"""msr_dense_search_deep on the GPU: row indices, keys and hit counts equal to the numpy references — the k-ordered
fmaf chain (tests/f32_chain.py) on an f32 handle, the exact product of dyadic inputs on an fp16 handle — at every k at
which deep_select_rows takes another instance, with duplicated rows, all-zero queries and k > n; the identities with
the search and with msr_dense_rank_rows; the refusals; the scratch kept on the handle."""
import numpy as np
import pytest

from tests.f32_chain import chain_scores, f32_keys, topk
from tests.select_ref import dyadic

pytestmark = pytest.mark.gpu

INVAL, RANGE = -1, -8
SHAPES = [(9000, 37, 1025), (9000, 37, 5000), (20517, 5, 16384), (3, 4, 2000)]   # (n, nq, k)
N_MAX, NQ = 20517, 37


@pytest.fixture(scope="module")
def m(built):
    import mllm_sparse_retrieval_amd as m

    return m


def _open(p, precision):
    from mllm_sparse_retrieval_amd.dense import DenseIndex

    return DenseIndex(p, device=0, precision=precision)


_REF = {}


def _f32_case():
    """(rows [N_MAX, 40], queries [NQ, 40], chain scores [NQ, N_MAX]), computed once: a score depends on its own row
    alone, so the first n columns of the first nq rows are the reference of every smaller shape."""
    if "f32" not in _REF:
        rng = np.random.default_rng(40)
        p = rng.standard_normal((N_MAX, 40)).astype(np.float32)
        q = rng.standard_normal((NQ, 40)).astype(np.float32)
        _REF["f32"] = (p, q, chain_scores(q, p))
    return _REF["f32"]


def _fp16_case():
    """Dyadic rows and queries (h = 64: every product and partial sum is exact in f32, in any order), rows i + 100 = rows
    i for the first hundred (ties the lower row wins), queries 1 and 3 all zero (the whole row is one tie class)."""
    if "fp16" not in _REF:
        rng = np.random.default_rng(64)
        p = dyadic(rng, (N_MAX, 64))
        p[100:200] = p[:100]
        q = dyadic(rng, (NQ, 64))
        q[1] = 0
        q[3] = 0
        _REF["fp16"] = (p, q, (q.astype(np.float64) @ p.astype(np.float64).T).astype(np.float32))
    return _REF["fp16"]


def _assert_equal(got, want):
    for g, w, name in zip(got, want, ("row indices", "keys", "hit counts")):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{len(bad)} {name} differ, first at {bad[0]}"


@pytest.mark.parametrize("n,nq,k", SHAPES)
def test_f32_against_the_chain(m, n, nq, k):
    p, q, scores = _f32_case()
    dix = _open(p[:n], "f32")
    try:
        got = dix.search_keys_deep(q[:nq], k)
        assert dix.last_ms[0] > 0 and dix.last_ms[1] > 0
        s, i = dix.search_deep(q[:nq], k)
    finally:
        dix.close()
    want = topk(scores[:nq, :n], k)
    _assert_equal(got, want)
    kk = min(k, n)
    assert (got[2] == kk).all() and s.dtype == np.float32 and i.dtype == np.int64
    assert (i[:, :kk] == want[0][:, :kk]).all() and (i[:, kk:] == -1).all() and np.isneginf(s[:, kk:]).all()
    assert (s[:, :kk] == np.take_along_axis(scores[:nq, :n], want[0][:, :kk].astype(np.int64), axis=1)).all()


@pytest.mark.parametrize("n,nq,k", SHAPES)
def test_fp16_against_the_exact_product(m, n, nq, k):
    p, q, scores = _fp16_case()
    assert (scores < 0).any() and (scores[1] == 0).all()
    dix = _open(p[:n], "fp16")
    try:
        got = dix.search_keys_deep(q[:nq], k)
    finally:
        dix.close()
    want = topk(scores[:nq, :n], k)
    _assert_equal(got, want)
    kk = min(k, n)
    assert (got[0][1, :kk] == np.arange(kk)).all()          # an all-zero query: rows 0 .. k - 1
    if n > 200:                                              # duplicated rows: the lower twin stands before the upper
        row = got[0][0, :kk].tolist()
        both = [(row.index(t), row.index(t + 100)) for t in range(100) if t in row and t + 100 in row]
        assert both and all(a < b and got[1][0, a] == got[1][0, b] for a, b in both)


@pytest.mark.parametrize("precision", ["f32", "fp16"])
def test_identities_with_search_and_rank_rows(m, precision):
    p, q, _ = _f32_case() if precision == "f32" else _fp16_case()
    n = 9000
    dix = _open(p[:n], precision)
    try:
        _assert_equal(dix.search_keys_deep(q, 1024), dix.search_keys(q, 1024))
        _assert_equal(dix.search_keys_deep(q, 7), dix.search_keys(q, 7))
        idx, key, cnt = dix.search_keys_deep(q, 5000)
        _assert_equal((idx[:, :1024], key[:, :1024]), dix.search_keys(q, 1024)[:2])
        rng = np.random.default_rng(3)
        cols = rng.integers(0, 5000, size=(NQ, 6))
        t_ptr = np.arange(NQ + 1, dtype=np.int64) * 6
        ranks, keys = dix.rank_rows(q, t_ptr, np.take_along_axis(idx, cols, axis=1).reshape(-1))
        assert (ranks == (cols + 1).reshape(-1)).all()
        assert (keys == np.take_along_axis(key, cols, axis=1).reshape(-1)).all()
    finally:
        dix.close()


def test_two_passes_at_the_first_k_above_2048():
    """The pass loop of the dense calls (DensePassLoop, csrc/msr_hybrid.hip) under the deep selection, over more than one
    pass: a pass's key rows stay at or below 256 MiB, so rb_max = max(1, 2^28 / (n_pad * 4 * 256)) blocks of 256 queries;
    once n_pad exceeds 2^17 rows that is 1 and 293 queries run as 256 + 37 (tests/test_dense_filtered.py walks the same
    passes). The queries are 40 distinct dyadic rows drawn by i % 40 (every score exact in any order), so a row lands in
    both passes; k = 2049 is the first k of the 8192-key instance. Expected: tests/deep_ref.py on the exact keys."""
    from tests import deep_ref as dr
    from tests.select_ref import f32_keys as exact_keys

    n, nq, h, k = 16 * 8192 + 37, 293, 8, 2049
    n_pad = -(-n // 8192) * 8192
    assert max(1, (256 << 20) // (n_pad * 4 * 256)) == 1 and max(1, (256 << 20) // ((n_pad - 8192) * 4 * 256)) == 2
    rng = np.random.default_rng(2049)
    p = dyadic(rng, (n, h))
    base = dyadic(rng, (40, h))
    pick = np.arange(nq) % 40
    assert len(set(pick[:256].tolist()) & set(pick[256:].tolist())) == 37          # rows scored in both passes
    K = exact_keys((base.astype(np.float64) @ p.astype(np.float64).T + 0.0).astype(np.float32)).astype(np.int64)
    assert (K > 0).all()
    want = dr.topk_rows(K, k)                                      # of the 40 distinct queries
    dix = _open(p, "f32")
    try:
        got = dix.search_keys_deep(base[pick], k)
    finally:
        dix.close()
    _assert_equal(got, tuple(w[pick] for w in want))
    assert (got[2] == k).all()


def test_scratch_stays_on_the_handle(m):
    p, q, _ = _f32_case()
    dix = _open(p[:9000], "f32")
    try:
        first = dix.search_keys_deep(q, 5000)
        before = dix.stats()
        again = dix.search_keys_deep(q, 5000)
        assert dix.stats() == before and before["device_allocs"] > 0
        _assert_equal(again, first)
    finally:
        dix.close()


def test_refusals(m):
    from mllm_sparse_retrieval_amd import _cabi

    p, q, _ = _f32_case()
    lib, ptr = _cabi.lib(), _cabi.ptr
    idx, key, cnt = np.zeros((2, 8), np.uint32), np.zeros((2, 8), np.uint32), np.zeros(2, np.int32)
    q16 = np.zeros((2, 64), np.float16)
    for precision, rows, q_ok, is_f32 in (("f32", p[:300], q[:2].copy(), 1), ("fp16", _fp16_case()[0][:300], q16, 0)):
        dix = _open(rows, precision)
        try:
            call = lambda f32, k: lib.msr_dense_search_deep(dix._h, ptr(q_ok), f32, 2, k, ptr(idx), ptr(key), ptr(cnt), None)
            assert call(1 - is_f32, 8) == INVAL and b"q_is_f32" in lib.msr_last_error()
            assert call(1 - is_f32, 0) == INVAL                       # the mismatch is reported before k
            for k in (0, -1, _cabi.MSR_DEEP_KMAX + 1):
                assert call(is_f32, k) == RANGE and b"MSR_DEEP_KMAX" in lib.msr_last_error()
            assert lib.msr_dense_search_deep(dix._h, ptr(q_ok), is_f32, 2, 8, None, ptr(key), ptr(cnt), None) == INVAL
            assert lib.msr_dense_search_deep(dix._h, None, is_f32, 2, 8, ptr(idx), ptr(key), ptr(cnt), None) == INVAL
            assert lib.msr_dense_search_deep(dix._h, ptr(q_ok), is_f32, -1, 8, ptr(idx), ptr(key), ptr(cnt), None) == INVAL
            assert lib.msr_dense_search_deep(dix._h, None, is_f32, 0, 8, ptr(idx), ptr(key), ptr(cnt), None) == 0   # nq == 0
            with pytest.raises(_cabi.MsrError):
                dix.search(q_ok if is_f32 else q16, 1025)             # the staged search still stops at MSR_KMAX
            assert call(is_f32, 8) == 0 and (cnt == 8).all()
        finally:
            dix.close()
