"""Dense half of the reference's hybrid search: flat inner product over passage vectors, top-`depth`.

Drop-in for tevatron's FaissFlatSearcher as src/search.py uses it:
    dense_retriever = FaissFlatSearcher(p_reps_0); dense_retriever.add(p_reps_0)        src/search.py:232-237
    all_scores, all_indices = retriever.batch_search(q_reps, depth, batch_size, quiet)  src/search.py:57
    (or retriever.search(q_reps, depth), src/search.py:59)
The reference's hybrid run keeps the vectors in fp16 on the GPU (co.useFloat16, src/search.py:257,267); so does this
class by default, with f32 accumulation on MFMA (msr_dense_search). Its other runs (no --use_gpu, src/arguments.py:63)
search a plain f32 IndexFlatIP on the CPU: precision="f32" is that search (msr_dense_search_f32), every score the
k-ordered fmaf chain of f32 inputs; hybrid_search_f32 is the hybrid search on such a handle. Ties in score are broken by
the lower row index.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

from ._cabi import MSR_KMAX, check, lib, ptr


def keys_to_f32(keys):
    """Inverse of the order-preserving f32 -> u32 map of the kernels (include/msr.h); key 0 (padding) -> -inf."""
    keys = np.asarray(keys, dtype=np.uint32)
    bits = np.where(keys & np.uint32(0x80000000), keys & np.uint32(0x7FFFFFFF), ~keys)
    out = bits.astype(np.uint32).view(np.float32).copy()
    out[keys == 0] = -np.inf
    return out


def _as_fp16_rows(x, dim=None, holder=None):
    """[rows, dim] matrix -> C-contiguous fp16 (round to nearest even), columns padded to a multiple of 32.
    `holder`: an object whose `_q16` attribute keeps the output buffer between calls (a fresh 200 MB array costs more in
    page faults than the conversion itself) — which makes the holder single-threaded, see DenseIndex.
    msr_f32_to_f16 rounds like numpy's astype(float16) for every non-NaN value (NaN payloads differ: F16C sets the
    quiet bit, numpy keeps the payload)."""
    x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError("expected a [rows, dim] matrix")
    h = x.shape[1]
    pad = (-h) % 32  # the GEMM steps K by 32; zero columns do not change inner products
    if dim is not None and h != dim:
        raise ValueError(f"dimension mismatch: {h} vs {dim}")
    if x.dtype == np.float32 and x.flags.c_contiguous and x.size >= (1 << 16):
        # (numpy converts ~0.2 G values/s on one core: for a big query matrix that is longer than the GPU search)
        x16 = getattr(holder, "_q16", None) if holder is not None and not pad else None
        if x16 is None or x16.shape != x.shape:
            x16 = np.empty(x.shape, dtype=np.float16)
            if holder is not None and not pad:
                holder._q16 = x16
        check(lib().msr_f32_to_f16(ptr(x), ptr(x16.view(np.uint16)), x.size, 0))
    else:
        x16 = x.astype(np.float16)
    if pad:
        x16 = np.concatenate([x16, np.zeros((x16.shape[0], pad), np.float16)], axis=1)
    return np.ascontiguousarray(x16)


PRECISIONS = ("fp16", "f32")


def _as_f32_rows(x, dim=None):
    """[rows, dim] matrix -> C-contiguous float32 (float64 rounds to nearest; float32 goes up as it is)."""
    x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError("expected a [rows, dim] matrix")
    if dim is not None and x.shape[1] != dim:
        raise ValueError(f"dimension mismatch: {x.shape[1]} vs {dim}")
    return np.ascontiguousarray(x, dtype=np.float32)


class DenseIndex:
    """Passage matrix resident in HBM: fp16 rows (precision="fp16", the default) or f32 rows (precision="f32").

    NOT thread-safe per handle (like every libmsr handle: one in-flight call per handle): the fp16 copy of the query
    matrix, the device scratch and the HIP stream all live on the handle and are reused by the next call. Threads that
    search concurrently each open their own DenseIndex."""

    def __init__(self, p_reps, device=0, precision="fp16"):
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {PRECISIONS}, got {precision!r}")
        self.precision = precision
        self._h = C.c_void_p()
        if precision == "f32":
            p32 = _as_f32_rows(p_reps)
            self.dim = p32.shape[1]
            self.n = p32.shape[0]
            check(lib().msr_dense_open_f32(ptr(p32), self.n, self.dim, int(device), C.byref(self._h)))
        else:
            p16 = _as_fp16_rows(p_reps)
            self.dim = np.asarray(p_reps).shape[1]
            self.n = p16.shape[0]
            check(lib().msr_dense_open(ptr(p16.view(np.uint16)), self.n, p16.shape[1], int(device), C.byref(self._h)))
        self.last_ms = (0.0, 0.0)
        self.last_rank_ms = (0.0, 0.0)

    def search_keys(self, q_reps, k):
        """-> (row indices uint32 [nq,k], order-preserving u32 score keys [nq,k], hit counts int32 [nq]) as the C-ABI
        returns them (include/msr.h: 0xFFFFFFFF / key 0 past the hit count)."""
        if self.precision == "f32":
            q = _as_f32_rows(q_reps, self.dim)
            fn, q_ptr = lib().msr_dense_search_f32, ptr(q)
        else:
            q = _as_fp16_rows(q_reps, self.dim, self)   # (consumed by the synchronous call below)
            fn, q_ptr = lib().msr_dense_search, ptr(q.view(np.uint16))
        nq = q.shape[0]
        idx = np.empty((nq, k), dtype=np.uint32)
        key = np.empty((nq, k), dtype=np.uint32)
        n = np.zeros(nq, dtype=np.int32)
        a, b = C.c_float(), C.c_float()
        check(fn(self._h, q_ptr, nq, int(k), ptr(idx), ptr(key), ptr(n), C.byref(a), C.byref(b)))
        self.last_ms = (a.value, b.value)
        return idx, key, n

    def search_keys_deep(self, q_reps, k):
        """search_keys for 1 <= k <= MSR_DEEP_KMAX (msr_dense_search_deep): the same GEMM, the exact top-k of every key
        row taken by the deep selection; bit-equal to search_keys for k <= MSR_KMAX."""
        if self.precision == "f32":
            q = _as_f32_rows(q_reps, self.dim)
            q_ptr, is_f32 = ptr(q), 1
        else:
            q = _as_fp16_rows(q_reps, self.dim, self)   # (consumed by the synchronous call below)
            q_ptr, is_f32 = ptr(q.view(np.uint16)), 0
        nq = q.shape[0]
        shape = (nq, max(int(k), 0))
        idx = np.empty(shape, dtype=np.uint32)
        key = np.empty(shape, dtype=np.uint32)
        n = np.zeros(nq, dtype=np.int32)
        ms = (C.c_float * 2)()
        check(lib().msr_dense_search_deep(self._h, q_ptr, is_f32, nq, int(k), ptr(idx), ptr(key), ptr(n), ms))
        self.last_ms = (ms[0], ms[1])
        return idx, key, n

    def search_deep(self, q_reps, k):
        """search for 1 <= k <= MSR_DEEP_KMAX: (scores float32 [nq,k], indices int64 [nq,k]), (-inf, -1) past the hits."""
        return self._scores_indices(*self.search_keys_deep(q_reps, k))

    def search_keys_filtered(self, q_reps, k, sets, q_set=None):
        """search_keys among the rows of each query's set (msr_dense_search_filtered). `sets`: bool [n_sets, n] or packed
        uint32 [n_sets, (n + 31) // 32] over ROW indices; q_set[i] in [-1, n_sets), -1 = unfiltered (None: no set, or one
        set for every query). Every row of the set is a hit: the hit count is min(k, |set|)."""
        from .filters import as_packed_sets, as_q_set

        if self.precision == "f32":
            q = _as_f32_rows(q_reps, self.dim)
            q_ptr, is_f32 = ptr(q), 1
        else:
            q = _as_fp16_rows(q_reps, self.dim, self)   # (consumed by the synchronous call below)
            q_ptr, is_f32 = ptr(q.view(np.uint16)), 0
        nq = q.shape[0]
        bits = as_packed_sets(sets, self.n)
        qs = as_q_set(q_set, nq, bits.shape[0])
        shape = (nq, max(int(k), 0))
        idx = np.empty(shape, dtype=np.uint32)
        key = np.empty(shape, dtype=np.uint32)
        n = np.zeros(nq, dtype=np.int32)
        ms = (C.c_float * 2)()
        check(lib().msr_dense_search_filtered(self._h, q_ptr, is_f32, nq, int(k), ptr(bits) if bits.shape[0] else None,
                                              int(bits.shape[0]), ptr(qs), ptr(idx), ptr(key), ptr(n), ms))
        self.last_ms = (ms[0], ms[1])
        return idx, key, n

    def search_filtered(self, q_reps, k, sets, q_set=None):
        """search among the rows of each query's set: (scores float32 [nq,k], indices int64 [nq,k]), (-inf, -1) past the
        hits (a set smaller than k)."""
        return self._scores_indices(*self.search_keys_filtered(q_reps, k, sets, q_set))

    def search(self, q_reps, k):
        """-> (scores float32 [nq,k], indices int64 [nq,k]); rows past the hit count hold (-inf, -1) like faiss."""
        return self._scores_indices(*self.search_keys(q_reps, k))

    @staticmethod
    def _scores_indices(idx, key, n):
        valid = np.arange(idx.shape[1])[None, :] < n[:, None]
        scores = np.where(valid, keys_to_f32(key), -np.inf).astype(np.float32)
        indices = np.where(valid, idx.astype(np.int64), -1)
        return scores, indices

    def rank_rows(self, q_reps, t_ptr, t_row, self_row=None):
        """Exact rank (1 = best; no depth limit) and score key of listed rows (msr_dense_rank_rows, include/msr.h): query i
        owns t_row[t_ptr[i]:t_ptr[i + 1]] (dense row indices, at most MSR_DENSE_RANK_MAX_TARGETS each, duplicates
        allowed); self_row[i] >= 0 names the row that does not count for query i (remove_query), whose own rank is 0.
        -> (ranks uint32, keys uint32), indexed like t_row; keys_to_f32(keys) are the scores."""
        if self.precision == "f32":
            q = _as_f32_rows(q_reps, self.dim)
            q_ptr, is_f32 = ptr(q), 1
        else:
            q = _as_fp16_rows(q_reps, self.dim, self)   # (consumed by the synchronous call below)
            q_ptr, is_f32 = ptr(q.view(np.uint16)), 0
        nq = q.shape[0]
        t_ptr = np.ascontiguousarray(t_ptr, dtype=np.int64)
        t_row = np.ascontiguousarray(t_row, dtype=np.uint32)
        if t_ptr.shape != (nq + 1,) or t_row.ndim != 1 or t_ptr[-1] != len(t_row):
            raise ValueError(f"malformed CSR target arrays: t_ptr needs {nq + 1} entries ending at len(t_row) = "
                             f"{t_row.size}, got shape {t_ptr.shape}")
        so = None if self_row is None else np.ascontiguousarray(self_row, dtype=np.int32)
        if so is not None and so.shape != (nq,):
            raise ValueError(f"self_row needs one entry per query ({nq}), got shape {so.shape}")
        ranks = np.zeros(len(t_row), dtype=np.uint32)
        keys = np.zeros(len(t_row), dtype=np.uint32)
        ms = (C.c_float * 2)()
        check(lib().msr_dense_rank_rows(self._h, q_ptr, is_f32, nq, ptr(t_ptr), ptr(t_row), ptr(so), ptr(ranks), ptr(keys),
                                        ms))
        self.last_rank_ms = (ms[0], ms[1])
        return ranks, keys

    def stats(self):
        """{'device_allocs': hipMalloc calls made for this handle's scratch, 'scratch_bytes': what it holds}."""
        out = np.zeros(4, dtype=np.uint64)
        check(lib().msr_dense_stats(self._h, ptr(out)))
        return dict(device_allocs=int(out[0]), scratch_bytes=int(out[1]))

    def close(self):
        if self._h:
            lib().msr_dense_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FaissFlatSearcher:
    """Same call shape as tevatron.retriever.searcher.FaissFlatSearcher (src/search.py:10,232-237,57-59).

    tevatron's own class is an f32 faiss IndexFlatIP; the reference searches that on the CPU unless --use_gpu clones
    it to the GPU with useFloat16 (src/search.py:254-270). precision="f32" matches the CPU run (the k-ordered fmaf chain
    of f32 inputs, include/msr.h); the default "fp16" matches the --use_gpu run the hybrid script uses."""

    def __init__(self, init_reps, device=0, precision="fp16", deep=False):
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {PRECISIONS}, got {precision!r}")
        self.deep = bool(deep)  # k > MSR_KMAX goes through DenseIndex.search_deep (up to MSR_DEEP_KMAX)
        self._dim = np.asarray(init_reps).shape[1]
        self._parts = []
        self._index = None
        self._device = device
        self.precision = precision

    def add(self, p_reps):
        p = np.asarray(p_reps, dtype=np.float32)
        if p.shape[1] != self._dim:
            raise ValueError("dimension mismatch")
        self._parts.append(p)
        if self._index is not None:
            self._index.close()
            self._index = None

    def _ready(self):
        if self._index is None:
            if not self._parts:
                raise RuntimeError("FaissFlatSearcher: no vectors were added")
            self._index = DenseIndex(np.concatenate(self._parts, axis=0), device=self._device,
                                     precision=self.precision)
        return self._index

    def _search(self, q_reps, k):
        ix = self._ready()
        return ix.search_deep(q_reps, k) if self.deep and k > MSR_KMAX else ix.search(q_reps, k)

    def search(self, q_reps, k):
        return self._search(q_reps, k)

    def search_filtered(self, q_reps, k, sets, q_set=None):
        """search among the rows of each query's set (DenseIndex.search_filtered): sets over ROW indices in add() order."""
        return self._ready().search_filtered(q_reps, k, sets, q_set)

    def batch_search(self, q_reps, k, batch_size, quiet=False):
        q = np.asarray(q_reps)
        self._ready()
        scores, indices = [], []
        for i in range(0, q.shape[0], max(int(batch_size), 1)):
            s, j = self._search(q[i:i + batch_size], k)
            scores.append(s)
            indices.append(j)
        return np.concatenate(scores, axis=0), np.concatenate(indices, axis=0)


def row_to_ordinal(sparse_index, lookup):
    """dense row r carries external id lookup[r] (the pkl's lookup list, src/search.py:61) -> sparse doc ordinal."""
    ord_of = {sparse_index.docid(o): o for o in range(sparse_index.n_docs)}
    return np.asarray([ord_of[str(x)] for x in lookup], dtype=np.uint32)


def hybrid_search(sparse_index, dense_index, q_ptr, q_term, q_w, q_reps, depth, k, alpha, row2ord, self_ord=None,
                  drop_df_eq_n=True):
    """Sparse top-`depth` + dense top-`depth` + min-max fusion (src/hybrid.py:32-53, weights [alpha, 1-alpha]) + top-k,
    all on the GPU. -> (doc ordinals uint32 [nq,k], fused scores float32 [nq,k], n [nq], kernel ms per stage)."""
    if getattr(dense_index, "precision", "fp16") != "fp16":
        raise ValueError("hybrid_search takes an fp16 DenseIndex (the reference's hybrid run uses --use_gpu, fp16 "
                         f"storage); this one holds {dense_index.precision} rows: search it with hybrid_search_f32")
    q16 = _as_fp16_rows(q_reps, dense_index.dim, dense_index)   # (consumed by the synchronous call below)
    return _hybrid_call(lib().msr_hybrid_search, sparse_index, dense_index, q_ptr, q_term, q_w, q16.view(np.uint16),
                        depth, k, alpha, row2ord, self_ord, drop_df_eq_n)


def hybrid_search_f32(sparse_index, dense_index, q_ptr, q_term, q_w, q_reps, depth, k, alpha, row2ord, self_ord=None,
                      drop_df_eq_n=True):
    """hybrid_search with the dense side in f32 (DenseIndex(precision="f32"): the reference's default, an f32
    IndexFlatIP without --use_gpu, src/arguments.py:63): every dense score is the k-ordered fmaf chain, bit-equal to
    DenseIndex.search_keys on the same handle. Same arguments and return value as hybrid_search."""
    if getattr(dense_index, "precision", "fp16") != "f32":
        raise ValueError("hybrid_search_f32 takes an f32 DenseIndex (precision=\"f32\"); this one holds "
                         f"{getattr(dense_index, 'precision', 'fp16')} rows: search it with hybrid_search")
    q32 = _as_f32_rows(q_reps, dense_index.dim)
    return _hybrid_call(lib().msr_hybrid_search_f32, sparse_index, dense_index, q_ptr, q_term, q_w, q32, depth, k, alpha,
                        row2ord, self_ord, drop_df_eq_n)


def _hybrid_call(fn, sparse_index, dense_index, q_ptr, q_term, q_w, q, depth, k, alpha, row2ord, self_ord, drop_df_eq_n):
    """One msr_hybrid_search / msr_hybrid_search_f32 call on query rows `q` already in the handle's precision."""
    from . import _cabi
    from ._cabi import MSR_F_DROP_DF_EQ_N

    q_ptr, q_term, q_w = _cabi.as_csr(q_ptr, q_term, q_w)
    nq = len(q_ptr) - 1
    if q.shape[0] != nq:
        raise ValueError("sparse and dense query counts differ")
    row2ord = np.ascontiguousarray(row2ord, dtype=np.uint32)
    if row2ord.shape != (dense_index.n,):
        raise ValueError(f"row2ord needs one ordinal per dense row ({dense_index.n}), got shape {row2ord.shape}")
    so = None if self_ord is None else np.ascontiguousarray(self_ord, dtype=np.int32)
    if so is not None and so.shape != (nq,):
        raise ValueError(f"self_ord needs one entry per query ({nq}), got shape {so.shape}")
    ords = np.empty((nq, k), dtype=np.uint32)
    sc = np.empty((nq, k), dtype=np.float32)
    n = np.zeros(nq, dtype=np.int32)
    ms = (C.c_float * 4)()
    check(fn(sparse_index._h, dense_index._h, ptr(q_ptr), ptr(q_term), ptr(q_w), ptr(q), nq, int(depth), int(k),
             float(alpha), MSR_F_DROP_DF_EQ_N if drop_df_eq_n else 0, ptr(row2ord), ptr(so), ptr(ords), ptr(sc), ptr(n), ms))
    return ords, sc, n, dict(sparse=ms[0], dense_gemm=ms[1], dense_select=ms[2], fusion=ms[3])


def hybrid_search_union(sparse_index, dense_index, q_ptr, q_term, q_w, q_reps, depth, alpha, row2ord, self_ord=None,
                        drop_df_eq_n=True, with_lists=True):
    """The whole fused union and both depth lists from ONE call (msr_hybrid_search_union): what the reference's hybrid run
    writes per query (src/search.py:455-461) — fuse() keeps every doc of either list, src/hybrid.py:32-53 — without a
    second sparse search or a second GEMM. fp16 or f32 follows dense_index.precision.
    -> (doc ordinals uint32 [nq, 2*depth] by fused score descending, fused scores float32, n [nq],
        src uint8 (bit 0: in the dense depth list, bit 1: in the sparse one), exact sparse scores uint32, dense scores
        float32, score_range float32 [nq, 4] = {dense max, dense min, sparse max, sparse min} of the unfiltered lists,
        kernel ms per stage); with_lists=False: None for src, the two score arrays and score_range (not downloaded)."""
    from . import _cabi
    from ._cabi import MSR_F_DROP_DF_EQ_N

    f32 = getattr(dense_index, "precision", "fp16") == "f32"
    if f32:
        q = _as_f32_rows(q_reps, dense_index.dim)
    else:
        q = _as_fp16_rows(q_reps, dense_index.dim, dense_index).view(np.uint16)   # (consumed by the synchronous call below)
    q_ptr, q_term, q_w = _cabi.as_csr(q_ptr, q_term, q_w)
    nq = len(q_ptr) - 1
    if q.shape[0] != nq:
        raise ValueError("sparse and dense query counts differ")
    row2ord = np.ascontiguousarray(row2ord, dtype=np.uint32)
    if row2ord.shape != (dense_index.n,):
        raise ValueError(f"row2ord needs one ordinal per dense row ({dense_index.n}), got shape {row2ord.shape}")
    so = None if self_ord is None else np.ascontiguousarray(self_ord, dtype=np.int32)
    if so is not None and so.shape != (nq,):
        raise ValueError(f"self_ord needs one entry per query ({nq}), got shape {so.shape}")
    w = 2 * max(int(depth), 0)
    ords = np.empty((nq, w), dtype=np.uint32)
    sc = np.empty((nq, w), dtype=np.float32)
    n = np.zeros(nq, dtype=np.int32)
    src = su = de = rng = None
    if with_lists:
        src, su = np.empty((nq, w), dtype=np.uint8), np.empty((nq, w), dtype=np.uint32)
        de, rng = np.empty((nq, w), dtype=np.float32), np.empty((nq, 4), dtype=np.float32)
    ms = (C.c_float * 4)()
    check(lib().msr_hybrid_search_union(sparse_index._h, dense_index._h, ptr(q_ptr), ptr(q_term), ptr(q_w), ptr(q),
                                        1 if f32 else 0, nq, int(depth), float(alpha),
                                        MSR_F_DROP_DF_EQ_N if drop_df_eq_n else 0, ptr(row2ord), ptr(so), ptr(ords), ptr(sc),
                                        ptr(n), ptr(src), ptr(su), ptr(de), ptr(rng), ms))
    return ords, sc, n, src, su, de, rng, dict(sparse=ms[0], dense_gemm=ms[1], dense_select=ms[2], fusion=ms[3])


def hybrid_sweep(sparse_index, dense_index, q_ptr, q_term, q_w, q_reps, depth, k, alphas, row2ord, self_ord=None,
                 drop_df_eq_n=True):
    """ONE hybrid scoring fused at every alpha of `alphas` (msr_hybrid_sweep): the union pass of hybrid_search_union runs
    once, its union stays on the device and is re-fused and re-ranked per alpha. Slice a is, bit for bit, the first k
    columns of hybrid_search_union(alpha=alphas[a]) and, for k <= MSR_KMAX, hybrid_search[_f32](alphas[a], k).
    fp16 or f32 follows dense_index.precision. 1 <= k <= 2 * depth, 1 <= len(alphas) <= MSR_SWEEP_MAX_ALPHAS, finite.
    -> (doc ordinals uint32 [A, nq, k], fused scores float32 [A, nq, k], n int32 [A, nq], kernel ms per stage: sparse,
        dense_gemm, dense_select, fusion (the union pass), sweep (the sweep kernels summed), groups (alpha groups launched))."""
    from . import _cabi
    from ._cabi import MSR_F_DROP_DF_EQ_N, MSR_SWEEP_MAX_ALPHAS

    f32 = getattr(dense_index, "precision", "fp16") == "f32"
    al = np.ascontiguousarray(alphas, dtype=np.float32)
    if al.ndim != 1 or not 1 <= al.size <= MSR_SWEEP_MAX_ALPHAS:
        raise ValueError(f"alphas needs 1 to MSR_SWEEP_MAX_ALPHAS = {MSR_SWEEP_MAX_ALPHAS} values in one dimension, got "
                         f"shape {al.shape}")
    if not np.isfinite(al).all():
        raise ValueError(f"alphas must be finite, got {al.tolist()}")
    depth, k = int(depth), int(k)
    if not 1 <= depth <= MSR_KMAX:
        raise ValueError(f"depth must be in [1, MSR_KMAX = {MSR_KMAX}], got {depth}")
    if not 1 <= k <= 2 * depth:
        raise ValueError(f"k must be in [1, 2 * depth = {2 * depth}], got {k}")
    if f32:
        q = _as_f32_rows(q_reps, dense_index.dim)
    else:
        q = _as_fp16_rows(q_reps, dense_index.dim, dense_index).view(np.uint16)   # (consumed by the synchronous call below)
    q_ptr, q_term, q_w = _cabi.as_csr(q_ptr, q_term, q_w)
    nq = len(q_ptr) - 1
    if q.shape[0] != nq:
        raise ValueError("sparse and dense query counts differ")
    row2ord = np.ascontiguousarray(row2ord, dtype=np.uint32)
    if row2ord.shape != (dense_index.n,):
        raise ValueError(f"row2ord needs one ordinal per dense row ({dense_index.n}), got shape {row2ord.shape}")
    so = None if self_ord is None else np.ascontiguousarray(self_ord, dtype=np.int32)
    if so is not None and so.shape != (nq,):
        raise ValueError(f"self_ord needs one entry per query ({nq}), got shape {so.shape}")
    ords = np.empty((al.size, nq, k), dtype=np.uint32)
    sc = np.empty((al.size, nq, k), dtype=np.float32)
    n = np.zeros((al.size, nq), dtype=np.int32)
    ms = (C.c_float * 6)()
    check(lib().msr_hybrid_sweep(sparse_index._h, dense_index._h, ptr(q_ptr), ptr(q_term), ptr(q_w), ptr(q),
                                 1 if f32 else 0, nq, depth, k, ptr(al), int(al.size),
                                 MSR_F_DROP_DF_EQ_N if drop_df_eq_n else 0, ptr(row2ord), ptr(so), ptr(ords), ptr(sc),
                                 ptr(n), ms))
    return ords, sc, n, dict(sparse=ms[0], dense_gemm=ms[1], dense_select=ms[2], fusion=ms[3], sweep=ms[4],
                             groups=int(ms[5]))


HybridDeep = namedtuple("HybridDeep", "ords scores n members src sparse_ords sparse_u32 sparse_n dense_ords dense dense_n "
                                      "score_range ms")


def hybrid_deep(sparse_index, dense_index, q_ptr, q_term, q_w, q_reps, depth, k, alphas, row2ord, self_ord=None,
                drop_df_eq_n=True, with_lists=True):
    """Deep hybrid search (msr_hybrid_deep): the fused union of two depth lists of up to MSR_DEEP_KMAX docs each, at every
    alpha of `alphas`, from ONE scoring. No candidate lists: both score rows stay on the device, both depth lists are exact
    row selections and fusion is an elementwise pass over the two rows (fuse_rows). For depth <= MSR_KMAX slice a at
    k = 2 * depth is, bit for bit, hybrid_search_union(alpha=alphas[a]). fp16 or f32 follows dense_index.precision.
    1 <= depth <= MSR_DEEP_KMAX, 1 <= k <= min(2 * depth, MSR_DEEP_KMAX), 1 <= len(alphas) <= MSR_SWEEP_MAX_ALPHAS, finite.
    -> HybridDeep: ords uint32 [A, nq, k], scores float32 [A, nq, k], n int32 [A, nq], members uint32 [nq] (the size of the
       union minus self_ord: above n where k cut the union), and with_lists: src uint8 [A, nq, k] (bit 0 dense, bit 1
       sparse), the sparse depth list (sparse_ords, sparse_u32 [nq, depth], sparse_n [nq]), the dense one (dense_ords,
       dense float32 scores, dense_n), score_range [nq, 4]; None for each otherwise. ms: kernel ms per stage (sparse,
       dense_gemm, depth_select, fuse_rows, fused_select) and passes."""
    return _hybrid_deep_call(sparse_index, dense_index, q_ptr, q_term, q_w, q_reps, depth, k, alphas, row2ord, None, self_ord,
                             drop_df_eq_n, with_lists)


def hybrid_deep_filtered(sparse_index, dense_index, q_ptr, q_term, q_w, q_reps, depth, k, alphas, row2ord, sets, q_set=None,
                         self_ord=None, drop_df_eq_n=True, with_lists=True):
    """hybrid_deep among the docs of each query's set (msr_hybrid_deep_filtered): both depth lists, the extremes and the
    fused union are those of an index that holds only the set's docs. `sets`: bool [n_sets, n_docs] or packed uint32
    [n_sets, (n_docs + 31) // 32] over doc ORDINALS (one bitmap serves both sides); q_set[i] in [-1, n_sets), -1 =
    unfiltered (None: no set, or one set for every query). A full set, -1 and no set give hybrid_deep bit for bit; an
    empty set gives n = members = 0 and empty depth lists. Same arguments otherwise and the same HybridDeep as
    hybrid_deep; ms gains `mask` (mask_key_rows, summed over the passes; 0 when no query is filtered)."""
    from .filters import as_packed_sets, as_q_set

    bits = as_packed_sets(sets, sparse_index.n_docs)
    qs = as_q_set(q_set, len(np.asarray(q_ptr)) - 1, bits.shape[0])
    return _hybrid_deep_call(sparse_index, dense_index, q_ptr, q_term, q_w, q_reps, depth, k, alphas, row2ord, (bits, qs),
                             self_ord, drop_df_eq_n, with_lists)


def _hybrid_deep_call(sparse_index, dense_index, q_ptr, q_term, q_w, q_reps, depth, k, alphas, row2ord, flt, self_ord,
                      drop_df_eq_n, with_lists):
    """One msr_hybrid_deep call, or with flt = (packed sets, q_set) one msr_hybrid_deep_filtered call."""
    from . import _cabi
    from ._cabi import MSR_DEEP_KMAX, MSR_F_DROP_DF_EQ_N, MSR_SWEEP_MAX_ALPHAS

    f32 = getattr(dense_index, "precision", "fp16") == "f32"
    al = np.ascontiguousarray(alphas, dtype=np.float32)
    if al.ndim != 1 or not 1 <= al.size <= MSR_SWEEP_MAX_ALPHAS:
        raise ValueError(f"alphas needs 1 to MSR_SWEEP_MAX_ALPHAS = {MSR_SWEEP_MAX_ALPHAS} values in one dimension, got "
                         f"shape {al.shape}")
    if not np.isfinite(al).all():
        raise ValueError(f"alphas must be finite, got {al.tolist()}")
    depth, k = int(depth), int(k)
    if not 1 <= depth <= MSR_DEEP_KMAX:
        raise ValueError(f"depth must be in [1, MSR_DEEP_KMAX = {MSR_DEEP_KMAX}], got {depth}")
    k_max = min(2 * depth, MSR_DEEP_KMAX)
    if not 1 <= k <= k_max:
        raise ValueError(f"k must be in [1, min(2 * depth, MSR_DEEP_KMAX) = {k_max}], got {k}")
    if f32:
        q = _as_f32_rows(q_reps, dense_index.dim)
    else:
        q = _as_fp16_rows(q_reps, dense_index.dim, dense_index).view(np.uint16)   # (consumed by the synchronous call below)
    q_ptr, q_term, q_w = _cabi.as_csr(q_ptr, q_term, q_w)
    nq = len(q_ptr) - 1
    if q.shape[0] != nq:
        raise ValueError("sparse and dense query counts differ")
    row2ord = np.ascontiguousarray(row2ord, dtype=np.uint32)
    if row2ord.shape != (dense_index.n,):
        raise ValueError(f"row2ord needs one ordinal per dense row ({dense_index.n}), got shape {row2ord.shape}")
    so = None if self_ord is None else np.ascontiguousarray(self_ord, dtype=np.int32)
    if so is not None and so.shape != (nq,):
        raise ValueError(f"self_ord needs one entry per query ({nq}), got shape {so.shape}")
    ords = np.empty((al.size, nq, k), dtype=np.uint32)
    sc = np.empty((al.size, nq, k), dtype=np.float32)
    n = np.zeros((al.size, nq), dtype=np.int32)
    members = np.zeros(nq, dtype=np.uint32)
    src = s_ord = s_u32 = s_n = d_ord = d_sc = d_n = rng = None
    if with_lists:
        src = np.empty((al.size, nq, k), dtype=np.uint8)
        s_ord, s_u32, s_n = np.empty((nq, depth), np.uint32), np.empty((nq, depth), np.uint32), np.zeros(nq, np.int32)
        d_ord, d_sc, d_n = np.empty((nq, depth), np.uint32), np.empty((nq, depth), np.float32), np.zeros(nq, np.int32)
        rng = np.zeros((nq, 4), dtype=np.float32)
    ms = (C.c_float * 7)()
    head = (sparse_index._h, dense_index._h, ptr(q_ptr), ptr(q_term), ptr(q_w), ptr(q), 1 if f32 else 0, nq, depth, k, ptr(al),
            int(al.size), MSR_F_DROP_DF_EQ_N if drop_df_eq_n else 0, ptr(row2ord), ptr(so))
    outs = (ptr(ords), ptr(sc), ptr(n), ptr(members), ptr(src), ptr(s_ord), ptr(s_u32), ptr(s_n), ptr(d_ord), ptr(d_sc),
            ptr(d_n), ptr(rng), ms)
    if flt is None:
        check(lib().msr_hybrid_deep(*head, *outs))
    else:
        bits, qs = flt
        check(lib().msr_hybrid_deep_filtered(*head, ptr(bits) if bits.shape[0] else None, int(bits.shape[0]), ptr(qs), *outs))
    times = dict(sparse=ms[0], dense_gemm=ms[1], depth_select=ms[2], fuse_rows=ms[3], fused_select=ms[4], passes=int(ms[5]))
    if flt is not None:
        times["mask"] = ms[6]
    return HybridDeep(ords, sc, n, members, src, s_ord, s_u32, s_n, d_ord, d_sc, d_n, rng, times)
