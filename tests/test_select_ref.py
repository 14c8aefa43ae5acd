"""CPU checks of the exact references in tests/select_ref.py against brute force, so that the GPU tests built on them
(tests/test_select_merge.py, tests/test_launch_splits.py) compare kernels with something known to be right."""
import numpy as np

from tests.select_ref import (NO_DOC, dense_topk_sparse_rows, dyadic, f32_keys, log1p_relu_f16, log1p_relu_f32,
                              merge_ref)


def test_merge_ref_against_sorted():
    rng = np.random.default_rng(0)
    for L, nq, k in [(1, 3, 1), (4, 5, 7), (9, 2, 30)]:
        ords = rng.permutation(L * nq * k).reshape(L, nq, k).astype(np.uint32)
        sc = rng.integers(0, 4, size=(L, nq, k)).astype(np.uint32)  # score 0 marks an empty slot
        n = rng.integers(-1, k + 2, size=(L, nq)).astype(np.int32)  # counts outside [0, k] are clamped
        o, s, cnt = merge_ref(ords, sc, n, k)
        for q in range(nq):
            items = sorted((-int(sc[l, q, j]), int(ords[l, q, j])) for l in range(L)
                           for j in range(min(max(int(n[l, q]), 0), k)) if sc[l, q, j])[:k]
            assert cnt[q] == len(items)
            assert [int(x) for x in o[q, : len(items)]] == [b for _, b in items]
            assert [int(x) for x in s[q, : len(items)]] == [-a for a, _ in items]
            assert (o[q, len(items):] == NO_DOC).all() and (s[q, len(items):] == 0).all()


def test_dense_topk_sparse_rows_against_full_matrix():
    rng = np.random.default_rng(1)
    n, h = 700, 16
    rows = np.unique(rng.integers(0, n, size=120))
    pr = dyadic(rng, (len(rows), h)) * (rng.random((len(rows), h)) < 0.3)
    pr[3] = pr[1]  # equal rows: ties to the lower row
    q = dyadic(rng, (9, h))
    q[0] = 0
    q[1] = 0
    q[1, 2] = 1.5
    P = np.zeros((n, h))
    P[rows] = pr
    full = q.astype(np.float64) @ P.T
    assert (full.astype(np.float32) == q @ P.astype(np.float32).T).all()  # dyadic inputs: f32 arithmetic is exact
    for k in (1, 10, 400, 700, 900):
        idx, val = dense_topk_sparse_rows(q, rows, pr, n, k)
        kk = min(k, n)
        order = np.lexsort((np.broadcast_to(np.arange(n), full.shape), -full), axis=1)[:, :kk]
        assert (idx == order).all(), k
        assert (val == np.take_along_axis(full, order, axis=1)).all()


def test_f32_keys_order():
    x = np.array([-np.inf, -2.0, -0.0, 0.0, 1e-30, 1.0, np.inf], dtype=np.float32)
    keys = f32_keys(x).astype(np.int64)
    assert (np.diff(keys) > 0).all() and (keys > 0).all()


def test_log1p_relu_references():
    # f32: the argument is the f32 sum 1 + relu(x); both f32 neighbours of the float64 log (what a faithfully rounded
    # logf may return) lie within the ulp
    rng = np.random.default_rng(2)
    x = np.concatenate([rng.standard_normal(100000) * 4, [-1.0, 0.0, 1e-8, 3e38]]).astype(np.float32)
    v, ulp = log1p_relu_f32(x)
    y = np.float32(1) + np.maximum(x, np.float32(0))
    assert (y.astype(np.float64) == 1 + np.maximum(x.astype(np.float64), 0)).mean() > 0.5  # (a rounded sum, often inexact)
    lo = v.astype(np.float32)
    hi = np.nextafter(lo, np.where(lo.astype(np.float64) < v, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    assert (np.abs(lo - v) <= ulp).all() and (np.abs(hi - v) <= ulp).all()
    assert (v[x <= 0] == 0).all()
    # f16: every positive finite half; rounding the f32 log to half agrees with the reference except on the
    # exemption list, which stays small
    xs = np.arange(0x0001, 0x7C00, dtype=np.uint16).view(np.float16)
    want, near = log1p_relu_f16(xs)
    y16 = np.float16(1) + xs
    via_f32 = np.log(y16.astype(np.float32)).astype(np.float16)
    assert (via_f32 == want)[~near].all()
    assert 0 < near.sum() <= 40, int(near.sum())
    assert (np.diff(want.astype(np.float64)) >= 0).all()  # monotone in x
