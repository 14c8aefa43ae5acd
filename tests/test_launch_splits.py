"""Host code that switches on size: the dense search's GEMM slices and query passes, and the three ways a small
msr_search_csr call moves its data. Expectations are exact references built here (tests/select_ref.py, the C oracle).

Dense search (csrc/msr_hybrid.hip):
    launch_dense_gemm / launch_dense_gemm_f32   doc blocks in slices of kMaxGridY (65 535) blocks: 128 x 65 535 docs
                                                for dense_scores / dense_scores_f32, 256 x 65 535 for dense_scores_256k
                                                (picked when h % 64 == 0 and the grid holds >= 256 blocks of 256 x 256)
    dense_search_impl                           queries in passes of qt = 256 rows once the score rows of 256 queries
                                                exceed 256 MB (n_pad > 262 144); pass q0 lands at out + q0 * k"""
import numpy as np
import pytest

from tests import helpers
from tests.select_ref import dense_topk_sparse_rows, dyadic, f32_keys

pytestmark = pytest.mark.gpu

SLICE = 65535  # kMaxGridY
NQ = 2 * 256 + 37  # three query passes of 256, 256 and 37 rows


def _dense_case(n, h, precision, boundary, seed):
    """P zero except in windows around the slice boundary, at the first and at the last rows; winners of half the
    queries planted just before the boundary, of the other half just past it; a row copied across the boundary and the
    first row copied to the last (equal scores: the lower row must win)."""
    rng = np.random.default_rng(seed)
    rows = np.unique(np.concatenate([np.arange(0, 300), np.arange(boundary - 700, boundary + 700),
                                     np.arange(n - 600, n)]))
    pr = dyadic(rng, (len(rows), h)) * (rng.random((len(rows), h)) < 0.3)
    q = dyadic(rng, (NQ, h))
    q[5::11] = 0  # zero queries: every score 0, the answer is rows 0 .. k-1
    hot = np.arange(6, NQ, 11)  # one-hot queries: few positive scores, then the run of exact zeros
    q[hot] = 0
    q[hot, hot % h] = 1.5
    at = {int(r): i for i, r in enumerate(rows)}
    planted = [i for i in range(NQ) if i % 11 not in (5, 6)][::2]
    for j, i in enumerate(planted):  # the best row a query can have: 2 * sum |q|
        r = boundary + j // 2 if j % 2 else boundary - 1 - j // 2
        pr[at[r]] = 2 * np.sign(q[i])
    pr[at[boundary]] = pr[at[boundary - 1]]
    pr[at[n - 1]] = pr[at[0]]
    P = np.zeros((n, h), dtype=np.float16 if precision == "fp16" else np.float32)
    P[rows] = pr
    return P, q, rows, pr


def _check_dense(P, q, rows, pr, precision, ks=(10, 1024)):
    from mllm_sparse_retrieval_amd.dense import DenseIndex

    n = P.shape[0]
    dix = DenseIndex(P, device=0, precision=precision)
    try:
        for k in ks:
            idx, key, cnt = dix.search_keys(q.astype(np.float16) if precision == "fp16" else q, k)
            w_idx, w_val = dense_topk_sparse_rows(q, rows, pr, n, k)
            assert (cnt == k).all()
            bad = np.argwhere(idx != w_idx)
            assert bad.size == 0, f"k={k}: {len(bad)} ids differ, first at {bad[0]}: {idx[tuple(bad[0])]} vs {w_idx[tuple(bad[0])]}"
            assert (key == f32_keys(w_val.astype(np.float32))).all(), f"k={k}: keys differ"
    finally:
        dix.close()


def test_dense_f32_gemm_slices_and_query_passes(built):
    # dense_scores_f32: a second doc slice of 5 000 docs (+ padding), a tile straddles the slice boundary
    n = 128 * SLICE + 5000
    _check_dense(*_dense_case(n, 8, "f32", 128 * SLICE, seed=1), "f32")


def test_dense_fp16_128_gemm_slices_and_query_passes(built):
    # dense_scores (128 x 128): h = 32 is not a multiple of 64, so `big` is false whatever the grid
    n = 128 * SLICE + 5000
    P, q, rows, pr = _dense_case(n, 32, "fp16", 128 * SLICE, seed=2)
    _check_dense(P, q, rows, pr, "fp16")


def test_dense_fp16_256k_gemm_slices_and_query_passes(built):
    # dense_scores_256k: h % 64 == 0, n_cover % 256 == 0 and (qn_pad / 256) * (n_cover / 256) >= 256 in every pass;
    # about 2 GB of P and 17 GB of score rows on the device
    n = 256 * SLICE + 3000
    P, q, rows, pr = _dense_case(n, 64, "fp16", 256 * SLICE, seed=3)
    _check_dense(P, q, rows, pr, "fp16", ks=(10, 1024))


# ------------------------------------------------------------------------------------------------ small calls
def test_search_csr_small_call_paths_agree(built, tmp_path):
    """msr_search_csr (csrc/msr_device.hip batch_create_impl, msr_batch_fetch) moves a call's data one of three ways:
        zero-copy   in and out blocks <= kZeroCopyBytes (64 KiB) and ntiles * nq <= kSmallMaxPairs (1024)
        staging     otherwise, through the pinned staging buffer (max(input, 1 MiB)), one copy each way
        plain       results larger than the staging buffer: hipMemcpy per array
    index.py keeps result buffers per (nq, k) for nq * k <= 1024. All of it must agree bit for bit with one resident
    batch and with the C oracle, in any order on one handle."""
    import mllm_sparse_retrieval_amd as m

    n_terms = 20000
    docs = m.synth_vectors(40000, 24, n_terms, seed=41)
    path = m.build_index_from_csr(str(tmp_path / "p.idx"), *docs, n_terms, tile_docs=4096)
    oix, _ = helpers.taat_oracle(docs, n_terms)
    qs = m.synth_vectors(110, 20, n_terms, seed=42)
    bp, bt, bw = m.synth_vectors(1, 17000, n_terms, seed=43)  # one query of 17 000 terms: a 136 KB input block

    def sub(csr, a, b):
        p, t, w = csr
        p = np.asarray(p, dtype=np.int64)
        return (p[a : b + 1] - p[a]), np.asarray(t[p[a] : p[b]], np.int32), np.asarray(w[p[a] : p[b]], np.int32)

    cases = {  # name -> (queries, k, way)
        "4x10": (sub(qs, 0, 4), 10, "zero-copy"),
        "2x10": (sub(qs, 4, 6), 10, "zero-copy"),
        "4x1024": (sub(qs, 0, 4), 1024, "zero-copy"),  # out block 3 x 4096 + 64 words = 49 KiB
        "103x9": (sub(qs, 0, 103), 9, "staging"),  # 10 tiles x 103 queries > 1024 pairs; nq * k = 927: cached buffers
        "big1x10": ((np.asarray(bp, np.int64), np.asarray(bt, np.int32), np.asarray(bw, np.int32)), 10, "staging"),
        "100x1024": (sub(qs, 0, 100), 1024, "plain"),  # 3 x 102 400 words of results > the 1 MiB staging buffer
    }
    with m.SparseIndex(path, device=0) as ix:
        assert ix.shard_ntiles == 10
        want = {}
        for name, (csr, k, way) in cases.items():
            b = ix.batch(*csr, k)
            b.search(k)
            want[name] = b.fetch()
            b.close()
            helpers.assert_same_results(want[name], oix.search(*csr, k, threads=8), k)
        order = ["4x10", "2x10", "4x10", "4x1024", "103x9", "4x10", "big1x10", "2x10", "100x1024", "4x10", "103x9",
                 "4x1024", "2x10"]
        kept = []
        for name in order:
            csr, k, way = cases[name]
            got = ix.search_csr(*csr, k)
            for g, w in zip(got, want[name]):
                assert g.dtype == w.dtype and g.shape == w.shape
                assert (g.view(np.uint32) == w.view(np.uint32)).all(), (name, way)
            kept.append((name, got))
        for name, got in kept:  # the cached buffers hand out copies: earlier results stay as they were
            for g, w in zip(got, want[name]):
                assert (g.view(np.uint32) == w.view(np.uint32)).all(), name
