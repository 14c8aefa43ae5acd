"""Exact ranks of listed rows on the dense route (msr_dense_rank_rows, DenseIndex.rank_rows, dense `search --ranks`):
ranks and keys equal to the numpy reference (tests/dense_rank_ref.py over the k-ordered fmaf chain) at the row-bound,
tile and target-group edges, the self rule, two passes, the link to the search on f32 and fp16 handles, refusals,
the scratch kept on the handle, and the CLI end to end."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.dense_rank_ref import f32_ranks, random_targets, ranks_from_keys, targets_csr
from tests.f32_chain import chain_scores, f32_keys

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVAL, RANGE = -1, -8
N_MAX, NQ = 9000, 130


@pytest.fixture(scope="module")
def m(built):
    import mllm_sparse_retrieval_amd as m

    return m


def _rows(rng, n, h, dup_every=0):
    x = rng.standard_normal((n, h)).astype(np.float32)
    if dup_every and n > dup_every:
        x[dup_every::dup_every] = x[0]  # bit-equal rows: score ties the lower row must win
    return x


_CHAIN = {}


def _chain(h):
    """(rows [N_MAX, h] with every 97th a copy of row 0, queries [NQ, h], chain keys [NQ, N_MAX]), computed once per h
    and never changed: a score depends on its own row alone, so the first n rows and columns are the reference of an
    index of n rows."""
    if h not in _CHAIN:
        rng = np.random.default_rng(500 + h)
        p, q = _rows(rng, N_MAX, h, dup_every=97), _rows(rng, NQ, h)
        _CHAIN[h] = (p, q, f32_keys(chain_scores(q, p)))
    return _CHAIN[h]


def _open(p, precision="f32"):
    from mllm_sparse_retrieval_amd.dense import DenseIndex

    return DenseIndex(p, device=0, precision=precision)


def _assert_exact(got, want):
    (ranks, keys), (w_ranks, w_keys) = got, want
    assert ranks.dtype == np.uint32 and keys.dtype == np.uint32
    bad = np.flatnonzero(keys != w_keys)
    assert bad.size == 0, f"{bad.size} keys differ, first at entry {bad[0]}: {keys[bad[0]]:#x} vs {w_keys[bad[0]]:#x}"
    bad = np.flatnonzero(ranks != w_ranks)
    assert bad.size == 0, f"{bad.size} ranks differ, first at entry {bad[0]}: {ranks[bad[0]]} vs {w_ranks[bad[0]]}"


@pytest.mark.parametrize("h", [1, 3, 100])
@pytest.mark.parametrize("n", [3, 5, 1021, 1024, 4096, 4097, 9000])
def test_f32_exact(m, n, h):
    p, q, keys = _chain(h)
    rng = np.random.default_rng(n * 1000 + h)
    lists = random_targets(rng, NQ, n)
    for i, t in enumerate(lists):  # planted: both twins of a tie, row 0, the last row
        if i % 3 == 0:
            t += [0, n - 1] + ([97, 194] if n > 194 else [])
    t_ptr, t_row = targets_csr(lists)
    dix = _open(p[:n])
    try:
        got = dix.rank_rows(q, t_ptr, t_row)
        assert dix.last_rank_ms[0] > 0 and dix.last_rank_ms[1] > 0
    finally:
        dix.close()
    _assert_exact(got, ranks_from_keys(keys[:, :n], t_ptr, t_row))


def test_target_group_edges(m):
    from mllm_sparse_retrieval_amd._cabi import MsrError

    n = 700
    p, q, keys = _chain(3)
    rng = np.random.default_rng(21)
    lists = [rng.integers(0, n, size=c).tolist() for c in (1, 8, 9, 63, 64, 0, 64, 7)]
    t_ptr, t_row = targets_csr(lists)
    dix = _open(p[:n])
    try:
        _assert_exact(dix.rank_rows(q[:8], t_ptr, t_row), ranks_from_keys(keys[:8, :n], t_ptr, t_row))
        lists[2] = rng.integers(0, n, size=65).tolist()
        with pytest.raises(MsrError) as e:
            dix.rank_rows(q[:8], *targets_csr(lists))
        assert e.value.code == RANGE and "MSR_DENSE_RANK_MAX_TARGETS" in str(e.value)
    finally:
        dix.close()


def test_self_rule(m):
    n, nq = 700, 40
    p, q, keys = _chain(3)
    keys = keys[:nq, :n]
    rng = np.random.default_rng(22)
    # rows 0, 97, 194, 291, ... are bit-equal: 194 is tied from below by 97 and from above by 291
    lists = [[194] + rng.integers(0, n, size=3).tolist() for _ in range(nq)]
    t_ptr, t_row = targets_csr(lists)
    best = np.argmax(keys.astype(np.int64), axis=1)  # (the first maximum: the row the search puts first)
    dix = _open(p[:n])
    try:
        free = dix.rank_rows(q[:nq], t_ptr, t_row)
        _assert_exact(free, ranks_from_keys(keys, t_ptr, t_row))
        _assert_exact(dix.rank_rows(q[:nq], t_ptr, t_row, np.full(nq, -1)), free)
        for self_row in (best, np.full(nq, 194), np.full(nq, 97), np.full(nq, 291),
                         np.where(np.arange(nq) % 2 == 0, -1, 97)):
            got = dix.rank_rows(q[:nq], t_ptr, t_row, self_row)
            _assert_exact(got, ranks_from_keys(keys, t_ptr, t_row, self_row))
            assert (free[0] >= got[0]).all() and (free[1] == got[1]).all()
    finally:
        dix.close()


def test_two_passes(m):
    # 9000 rows -> 16384-column score rows -> 4096 queries per pass (pick_row_blocks: 16 row blocks), so 4200 queries
    # are two passes; the queries repeat 300 distinct rows, whose chain keys are the reference whatever the batch
    n, h, nq = 9000, 2, 4200
    rng = np.random.default_rng(23)
    p, qu = _rows(rng, n, h, dup_every=97), _rows(rng, 300, h)
    inv = rng.integers(0, 300, size=nq)
    q = qu[inv]
    lists = [rng.integers(0, n, size=2).tolist() for _ in range(nq)]
    lists[4095] = [n - 1]
    lists[4096] = [0, 97, 8999]
    t_ptr, t_row = targets_csr(lists)
    self_row = np.where(np.arange(nq) % 5 == 0, rng.integers(0, n, size=nq), -1)
    keys = f32_keys(chain_scores(qu, p))[inv]
    dix = _open(p)
    try:
        _assert_exact(dix.rank_rows(q, t_ptr, t_row, self_row), ranks_from_keys(keys, t_ptr, t_row, self_row))
    finally:
        dix.close()


def _assert_link(idx, key, ranks, keys, t_ptr, t_row, k):
    """Every listed row with rank <= k sits at column rank - 1 of the search at k with the same key, the others are
    absent."""
    seen_in = seen_out = 0
    for i in range(len(t_ptr) - 1):
        for e in range(int(t_ptr[i]), int(t_ptr[i + 1])):
            t, r = int(t_row[e]), int(ranks[e])
            assert r >= 1
            if r <= k:
                assert idx[i, r - 1] == t and key[i, r - 1] == keys[e], (i, t, r)
                seen_in += 1
            else:
                assert t not in idx[i], (i, t, r)
                seen_out += 1
    assert seen_in and seen_out


def _link_targets(rng, idx, n):
    """Per query: random rows, the search's first and last column, and a row the search does not return."""
    lists = random_targets(rng, idx.shape[0], n)
    for i, t in enumerate(lists):
        absent = np.setdiff1d(np.arange(n), idx[i])
        t += [int(idx[i, 0]), int(idx[i, -1]), int(absent[rng.integers(0, len(absent))])]
    return targets_csr(lists)


def test_link_to_the_search_f32(m):
    n, h, k = 9000, 100, 1000
    rng = np.random.default_rng(24)
    p, q = _rows(rng, n, h, dup_every=97), _rows(rng, 300, h)
    dix = _open(p)
    try:
        idx, key, cnt = dix.search_keys(q, k)
        assert (cnt == k).all()
        t_ptr, t_row = _link_targets(rng, idx, n)
        ranks, keys = dix.rank_rows(q, t_ptr, t_row)
        _assert_link(idx, key, ranks, keys, t_ptr, t_row, k)
        # batch invariance: a 7-query slice ranked in a call of its own
        a, b = 131, 138
        sl_ptr = t_ptr[a:b + 1] - t_ptr[a]
        sl = slice(int(t_ptr[a]), int(t_ptr[b]))
        _assert_exact(dix.rank_rows(q[a:b], sl_ptr, t_row[sl]), (ranks[sl], keys[sl]))
    finally:
        dix.close()


def test_fp16_whole_row(m):
    n, h, nq = 1000, 64, 130
    rng = np.random.default_rng(25)
    p, q = _rows(rng, n, h, dup_every=97), _rows(rng, nq, h)
    dix = _open(p, "fp16")
    try:
        idx, key, cnt = dix.search_keys(q, n)
        assert (cnt == n).all() and (np.sort(idx, axis=1) == np.arange(n)).all()
        full = np.zeros((nq, n), dtype=np.uint32)  # the handle's own keys, by row
        np.put_along_axis(full, idx.astype(np.int64), key, axis=1)
        lists = random_targets(rng, nq, n)
        for i, t in enumerate(lists):
            t += [0, 97, 194, n - 1]
        t_ptr, t_row = targets_csr(lists)
        self_row = np.where(np.arange(nq) % 2 == 0, 97, -1)
        _assert_exact(dix.rank_rows(q, t_ptr, t_row), ranks_from_keys(full, t_ptr, t_row))
        _assert_exact(dix.rank_rows(q, t_ptr, t_row, self_row), ranks_from_keys(full, t_ptr, t_row, self_row))
    finally:
        dix.close()


def test_fp16_link_to_the_search(m):
    n, h, nq, k = 9000, 64, 130, 1000
    rng = np.random.default_rng(26)
    p, q = _rows(rng, n, h, dup_every=97), _rows(rng, nq, h)
    dix = _open(p, "fp16")
    try:
        idx, key, cnt = dix.search_keys(q, k)
        t_ptr, t_row = _link_targets(rng, idx, n)
        ranks, keys = dix.rank_rows(q, t_ptr, t_row)  # the same query matrix: the same passes and GEMM instance
        _assert_link(idx, key, ranks, keys, t_ptr, t_row, k)
    finally:
        dix.close()


def _raw(L, dix, q, is_f32, nq, t_ptr, t_row, self_row=None, ms=None):
    from mllm_sparse_retrieval_amd._cabi import ptr

    n = 0 if t_row is None else len(t_row)
    ranks, keys = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
    return L.msr_dense_rank_rows(dix._h, ptr(q), is_f32, nq, ptr(t_ptr), ptr(t_row), ptr(self_row), ptr(ranks), ptr(keys), ms)


def test_refusals_and_empties(m):
    from mllm_sparse_retrieval_amd import _cabi

    L = _cabi.lib()
    rng = np.random.default_rng(27)
    n, nq = 50, 4
    p, q = _rows(rng, n, 64), _rows(rng, nq, 64)
    q16 = q.astype(np.float16)
    t_ptr, t_row = targets_csr([[1], [2, 3], [], [49]])
    i32 = lambda *v: np.array(v, np.int32)  # noqa: E731
    d32, d16 = _open(p), _open(p, "fp16")
    try:
        assert _raw(L, d32, q16, 0, nq, t_ptr, t_row) == INVAL and b"msr_dense_open_f32" in L.msr_last_error()
        assert _raw(L, d16, q, 1, nq, t_ptr, t_row) == INVAL and b"msr_dense_open" in L.msr_last_error()
        assert _raw(L, d32, q, 1, nq, t_ptr, np.array([1, 2, 3, n], np.uint32)) == RANGE       # a row >= n
        assert _raw(L, d32, q, 1, nq, t_ptr, t_row, i32(-1, 0, n, -1)) == RANGE                # a self_row >= n
        assert _raw(L, d32, q, 1, nq, np.array([0, 2, 1, 3, 4], np.int64), t_row) == INVAL     # t_ptr decreases
        assert _raw(L, d32, q, 1, nq, np.array([1, 1, 3, 3, 4], np.int64), t_row) == INVAL     # does not start at 0
        assert _raw(L, d32, q, 1, -1, t_ptr, t_row) == INVAL
        assert _raw(L, d32, None, 1, nq, t_ptr, t_row) == INVAL
        with pytest.raises(ValueError):
            d32.rank_rows(q, t_ptr[:-1], t_row)
        with pytest.raises(ValueError):
            d32.rank_rows(q, t_ptr, t_row[:-1])
        with pytest.raises(ValueError):
            d32.rank_rows(q, t_ptr, t_row, [1, 2])
        before = d32.stats()
        for dix, qq, f in ((d32, q, 1), (d16, q16, 0)):
            ms = (ctypes.c_float * 2)(7.0, 7.0)
            assert _raw(L, dix, qq, f, 0, np.zeros(1, np.int64), None, ms=ms) == 0 and tuple(ms) == (0.0, 0.0)
            ms = (ctypes.c_float * 2)(7.0, 7.0)
            assert _raw(L, dix, qq, f, nq, np.zeros(nq + 1, np.int64), None, i32(-1, 3, -1, 0), ms=ms) == 0
            assert tuple(ms) == (0.0, 0.0)
        assert d32.stats() == before  # (no launch, no scratch)
        r, k = d32.rank_rows(q, np.zeros(nq + 1, np.int64), np.zeros(0, np.uint32))
        assert r.shape == (0,) and k.shape == (0,) and d32.last_rank_ms == (0.0, 0.0)
        # ... and the valid call on both handles
        _assert_exact(d32.rank_rows(q, t_ptr, t_row, i32(-1, 3, 0, 49)), f32_ranks(q, p, t_ptr, t_row, i32(-1, 3, 0, 49)))
        r, k = d16.rank_rows(q, t_ptr, t_row)
        assert ((r >= 1) & (r <= n)).all()
    finally:
        d32.close()
        d16.close()


def test_scratch_stays_on_the_handle(m):
    rng = np.random.default_rng(28)
    p, q = _rows(rng, 5000, 64), _rows(rng, 600, 64)
    t_ptr, t_row = targets_csr(random_targets(rng, 600, 5000, lo=1))
    dix = _open(p)
    try:
        a = dix.rank_rows(q, t_ptr, t_row)
        st = dix.stats()
        assert st["device_allocs"] > 0
        b = dix.rank_rows(q, t_ptr, t_row)
        assert dix.stats() == st
        _assert_exact(b, a)
    finally:
        dix.close()


def _run_cli(*args, cwd):
    r = subprocess.run([sys.executable, "-m", "mllm_sparse_retrieval_amd", *args], cwd=cwd, capture_output=True,
                       text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.mark.parametrize("mode", ["f32", "f32_remove_query", "fp16"])
def test_cli_dense_ranks(m, tmp_path, mode):
    import pickle

    from mllm_sparse_retrieval_amd.cli import normalize_rows
    from mllm_sparse_retrieval_amd.dense import keys_to_f32
    from mllm_sparse_retrieval_amd.ranks import rank_metrics

    rng = np.random.default_rng(29)
    n, h, nq = 60, 8, 12
    p = _rows(rng, n, h)
    qv = (p[:nq] + 0.1 * rng.standard_normal((nq, h))).astype(np.float32)  # query i looks like row i, which has ITS id
    target = [(7 * i + 3) % n for i in range(nq)]  # (never row i itself)
    target[0] = 0                  # ... but for query 0: its own row, rank 1, or 0 under --remove_query
    for i in (2, 5, 7):
        qv[i] -= 3 * p[target[i]]  # judged row far below --depth 5
    target[9] = 999                # judged id without a dense row
    dense = tmp_path / "dense"
    dense.mkdir()
    with open(dense / "corpus_0.pkl", "wb") as f:
        pickle.dump((p, [str(i) for i in range(n)]), f)
    with open(dense / "query.pkl", "wb") as f:
        pickle.dump((qv, [str(i) for i in range(nq)]), f)
    with open(tmp_path / "qrels.csv", "w") as f:
        f.write("imgid,filename,caption,sentid\n")
        for i in range(nq):
            f.write(f"{target[i]},{target[i]}.jpg,,{i}\n")
    remove = mode == "f32_remove_query"
    lists = [[t] if t < n else [] for t in target]
    t_ptr, t_row = targets_csr(lists)
    self_row = np.arange(nq) if remove else None
    q = normalize_rows(qv)
    if mode == "fp16":
        dix = _open(p, "fp16")
        try:
            idx, key, _ = dix.search_keys(q, n)
        finally:
            dix.close()
        full = np.zeros((nq, n), dtype=np.uint32)
        np.put_along_axis(full, idx.astype(np.int64), key, axis=1)
    else:
        full = f32_keys(chain_scores(q, p))
    w_ranks, w_keys = ranks_from_keys(full, t_ptr, t_row, self_row)
    assert (w_ranks > 5).sum() >= 3  # beyond the search depth
    want = rank_metrics(w_ranks, t_ptr, n)
    save = tmp_path / "runs"
    text = _run_cli("search", "--passage_reps", str(dense), "--depth", "5", "--qrels", str(tmp_path / "qrels.csv"),
                    "--query_type", "text", "--save_dir", str(save), "--ranks",
                    *(["--remove_query"] if remove else []), *(["--use_gpu"] if mode == "fp16" else []), cwd=str(tmp_path))
    assert sorted(os.listdir(save)) == ["dense.ranks.tsv", "dense.trec"]
    line = [x for x in text.splitlines() if x.startswith("Dense exact ranks:")]
    assert len(line) == 1 and "Sparse exact ranks" not in text
    rc = want["recall"]
    assert line[0] == ("Dense exact ranks: r@1 {}, r@5 {}, r@10 {}, r@100 {}, r@200 {}, mrr {}, medr {}, meanr {}, "
                       "unranked {}, missing 1".format(rc[1], rc[5], rc[10], rc[100], rc[200], want["mrr"], want["medr"],
                                                       want["meanr"], want["n_unranked"]))
    w_scores = keys_to_f32(w_keys)
    rows = [x.split("\t") for x in open(save / "dense.ranks.tsv").read().splitlines()]
    assert len(rows) == nq
    e = 0
    for i, (qid, docid, rank, score) in enumerate(rows):
        assert qid == str(i) and docid == str(target[i])
        if target[i] >= n:
            assert (rank, score) == ("-1", "0")
            continue
        assert int(rank) == w_ranks[e] and np.float32(float(score)) == w_scores[e] and float(score) == float(w_scores[e])
        e += 1
    if remove:
        mine = [i for i in range(nq) if target[i] == i]
        assert all(rows[i][2] == "0" for i in mine)
