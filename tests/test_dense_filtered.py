"""msr_dense_search_filtered on the GPU against numpy: dyadic rows and queries (tests/select_ref.py), so every score and
therefore every key is exact in any summation order, masked and ranked by tests/filter_ref.py. Exact equality of row
indices, keys and hit counts on fp16 (h = 32) and f32 (h = 8) handles of 2 * 4096 + 37 rows (two 8192-row tiles, the last
ragged) with the named sets plus two that sit on the 8192-row tile edge, at every k at which the selection takes another
path; k above |set|; rows duplicated across a set boundary; two passes of queries whose q_set differs between the passes;
the identities with the search and the deep search; the refusals in their order; the scratch kept on the handle."""
import numpy as np
import pytest

from tests import filter_ref as fr
from tests.select_ref import dyadic, f32_keys

pytestmark = pytest.mark.gpu

INVAL, RANGE = -1, -8
N, NQ, TILE = 2 * 4096 + 37, 70, 8192          # msr_dense_open: 8192-row tiles above 4096 rows
KS = [1, 10, 64, 65, 512, 513, 1024]
PREC = pytest.mark.parametrize("precision", ["fp16", "f32"])
H = {"fp16": 32, "f32": 8}


@pytest.fixture(scope="module")
def m(built):
    import mllm_sparse_retrieval_amd as m

    return m


def _open(p, precision):
    from mllm_sparse_retrieval_amd.dense import DenseIndex

    return DenseIndex(p, device=0, precision=precision)


def keys_of(q, p):
    """u32 keys of the exact scores (float64 product of dyadic inputs, -0 made +0 as an accumulator started at +0 gives)."""
    s = (q.astype(np.float64) @ p.astype(np.float64).T + 0.0).astype(np.float32)
    return f32_keys(s).astype(np.int64)


def sets_of(n):
    """The eight named sets (edges at 4096) + rows of tile 1 only (tile 0 exits early) + [5, 8195) across the tile edge."""
    member, words = fr.named_sets(n, 4096)
    o = np.arange(n)
    extra = np.stack([o >= TILE, (o >= 5) & (o < TILE + 3)])
    return np.concatenate([member, extra]), np.concatenate([words, fr.pack(extra)])


_CASE = {}


def case(precision):
    if precision not in _CASE:
        rng = np.random.default_rng(H[precision])
        p = dyadic(rng, (N, H[precision]))
        q = dyadic(rng, (NQ, H[precision]))
        # rows 4 .. 7 are one row, the best of query 0: duplicates on both sides of the edges of `span` ([5, 4099)) and of
        # `even`; 4098 / 4099 and 8191 / 8192 are twins across the other edges
        p[4:8] = 2.0
        q[0] = 2.0
        p[4099] = p[4098]
        p[8192] = p[8191]
        q[1] = 0                                  # an all-zero query: every row ties, the lowest member rows win
        member, words = sets_of(N)
        K = keys_of(q, p)
        assert (K > 0).all()
        _CASE[precision] = dict(p=p, q=q, K=K, member=member, words=words, refs={})
    return _CASE[precision]


@pytest.fixture(scope="module", params=["fp16", "f32"])
def opened(m, request):
    c = case(request.param)
    dix = _open(c["p"], request.param)
    yield c, dix
    dix.close()


def ref_of(c, q_set):
    key = tuple(np.asarray(q_set).tolist())
    if key not in c["refs"]:
        c["refs"][key] = fr.masked_topk(c["K"], c["member"], q_set, 1024)
    return c["refs"][key]


def compare(got, want):
    for g, w, name in zip(got, want, ("row indices", "keys", "hit counts")):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{len(bad)} {name} differ, first at {bad[0]}"


@pytest.mark.parametrize("k", KS)
def test_one_call_mixes_all_sets(opened, k):
    c, dix = opened
    q_set = ((np.arange(NQ) * 4) % 11 - 1).astype(np.int32)
    assert set(q_set.tolist()) == set(range(-1, 10))
    got = dix.search_keys_filtered(c["q"], k, c["words"], q_set)
    compare(got, fr.cut(ref_of(c, q_set), k))
    sizes = np.where(q_set >= 0, c["member"].sum(axis=1)[np.maximum(q_set, 0)], N)
    assert (got[2] == np.minimum(k, sizes)).all()                # every row of the set is a hit: out_n = min(k, |set|)
    assert dix.last_ms[0] > 0 and dix.last_ms[1] > 0


@pytest.mark.parametrize("s", range(10), ids=fr.SET_NAMES + ("tile1_8192", "span_8192"))
def test_every_query_on_one_set(opened, s):
    c, dix = opened
    q_set = np.full(NQ, s, dtype=np.int32)
    ref = ref_of(c, q_set)
    size = int(c["member"][s].sum())
    for k in (10, 512, 513, 1024):
        got = dix.search_keys_filtered(c["q"], k, c["words"], q_set)
        compare(got, fr.cut(ref, k))
        assert (got[2] == min(k, size)).all()                    # k > |set| gives out_n = |set| (empty, last, 37 rows ...)
        assert (got[0][:, min(k, size):] == 0xFFFFFFFF).all() and (got[1][:, min(k, size):] == 0).all()
    s_f, i_f = dix.search_filtered(c["q"], 64, c["words"], q_set)
    kk = min(64, size)
    assert s_f.dtype == np.float32 and i_f.dtype == np.int64
    assert (i_f[:, :kk] == ref[0][:, :kk]).all() and (i_f[:, kk:] == -1).all() and np.isneginf(s_f[:, kk:]).all()


def test_duplicates_across_a_set_boundary(opened):
    """Rows 4 .. 7 are equal and the best of query 0: among equal MEMBERS the lower row wins, a non-member twin is out."""
    c, dix = opened
    for name, first in (("full", [4, 5, 6, 7]), ("span", [5, 6, 7]), ("even", [4, 6]), ("full_garbage", [4, 5, 6, 7])):
        s = fr.SET_NAMES.index(name)
        idx, key, n = dix.search_keys_filtered(c["q"][:2], 10, c["words"], np.full(2, s, np.int32))
        assert idx[0, :len(first)].tolist() == first and len(set(key[0, :len(first)].tolist())) == 1, name
        assert key[0, len(first)] < key[0, 0]
        assert idx[1].tolist() == np.flatnonzero(c["member"][s])[:10].tolist()       # the all-zero query: lowest member rows
    # twins across the edges of span ([5, 4099): 4098 in, 4099 out) and of the 8192-row tile (8191 / 8192)
    span = fr.SET_NAMES.index("span")
    idx, key, n = dix.search_keys_filtered(c["q"], 1024, c["words"], np.full(NQ, span, np.int32))
    assert not (idx == 4099).any() and not (idx == 4).any()
    idx, key, n = dix.search_keys_filtered(c["q"], 1024, c["words"], np.full(NQ, 1, np.int32))
    for lo, hi in ((4098, 4099), (8191, 8192)):
        both = [(r.tolist().index(lo), r.tolist().index(hi)) for r in idx if lo in r and hi in r]
        assert both and all(b == a + 1 for a, b in both), (lo, hi)            # equal keys: adjacent, the lower row first


def test_identities_with_search_and_deep(opened):
    c, dix = opened
    full, garbage = fr.SET_NAMES.index("full"), fr.SET_NAMES.index("full_garbage")
    for k in (10, 513, 1024):
        plain = dix.search_keys(c["q"], k)
        for sets, q_set in ((c["words"], np.full(NQ, full)), (c["words"], np.full(NQ, garbage)), (c["words"], np.full(NQ, -1)),
                            (c["words"][full:full + 1], None), (c["words"][:0], None)):
            for a, b in zip(dix.search_keys_filtered(c["q"], k, sets, q_set), plain):     # bit-equal, padding included
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    deep_i, deep_k, deep_n = dix.search_keys_deep(c["q"], N)                  # the exact ranking of every row
    assert (deep_n == N).all()
    k = 1024
    for s in (4, 5, 6, 9):
        both = np.stack([c["member"][s], ~c["member"][s]])
        for side in (0, 1):
            idx, key, n = dix.search_keys_filtered(c["q"], k, both, np.full(NQ, side, np.int32))
            for i in range(NQ):
                keep = both[side][deep_i[i]]
                want = deep_i[i][keep][:k]
                assert n[i] == len(want) and (idx[i, :n[i]] == want).all() and (key[i, :n[i]] == deep_k[i][keep][:k]).all()


def test_two_passes_with_different_q_sets(m):
    """The dense search cuts a batch into passes of queries (dense_passes, csrc/msr_hybrid.hip): a pass's key rows stay
    at or below 256 MiB, so rb_max = max(1, 2^28 / (n_pad * 4 * 256)) blocks of 256 queries; once n_pad exceeds 2^17 =
    131 072 rows that is 1 and 293 queries run as 256 + 37. q_set is indexed by the query of the CALL: a kernel that
    indexed it by the query of the pass would give queries 256 .. 292 the sets of queries 0 .. 36, which differ here."""
    n, nq, h = 16 * 8192 + 37, 293, 8
    n_pad = -(-n // 8192) * 8192
    assert max(1, (256 << 20) // (n_pad * 4 * 256)) == 1 and max(1, (256 << 20) // ((n_pad - 8192) * 4 * 256)) == 2
    rng = np.random.default_rng(293)
    p = dyadic(rng, (n, h))
    base = dyadic(rng, (40, h))
    o = np.arange(n)
    member = np.stack([rng.random(n) < 0.5, (o >= 5) & (o < 8192 + 3), o >= 15 * 8192])
    K = keys_of(base, p)
    pick, q_set = np.arange(nq) % 40, (np.arange(nq) % 3).astype(np.int32)
    assert (q_set[256:] != q_set[:37]).all()
    combos = {(int(a), int(b)) for a, b in zip(pick, q_set)}                   # 120 distinct (query, set) rows
    ref = {}
    for s in range(3):
        rows = sorted(a for a, b in combos if b == s)
        idx, key, cnt = fr.masked_topk(K[rows], member, np.full(len(rows), s), 100)
        ref.update({(a, s): (idx[j], key[j], cnt[j]) for j, a in enumerate(rows)})
    dix = _open(p, "f32")
    try:
        idx, key, cnt = dix.search_keys_filtered(base[pick], 100, member, q_set)
        before = dix.stats()
        again = dix.search_keys_filtered(base[pick], 100, member, q_set)
        assert dix.stats() == before and before["device_allocs"] > 0           # the scratch stays with the handle
    finally:
        dix.close()
    compare(again, (idx, key, cnt))
    for i in range(nq):
        w = ref[(int(pick[i]), int(q_set[i]))]
        assert cnt[i] == w[2] == 100 and (idx[i] == w[0]).all() and (key[i] == w[1]).all(), i


def test_calls_interleaved_on_one_handle(m):
    """search, search_deep, search_filtered and rank_rows share the query and score scratch of the handle (S_Q, S_S), the
    plain and the filtered search also their list and result slots, and all four one pass loop (csrc/msr_hybrid.hip).
    Interleaved on one handle each call returns what it returns alone on a fresh handle and what the references give;
    the first search repeated at the end returns the same again; a second round allocates nothing."""
    from tests import deep_ref as dr
    from tests import dense_rank_ref as drr

    c = case("f32")
    rng = np.random.default_rng(5)
    q = dyadic(rng, (260, H["f32"]))
    K = keys_of(q, c["p"])
    assert (K > 0).all()
    member = c["member"][[4, 5]]                                             # even, span
    q_set = (np.arange(7) % 3 - 1).astype(np.int32)
    t_ptr, t_row = drr.targets_csr(drr.random_targets(rng, 20, N, lo=0, hi=5))
    calls = [("search", lambda d: d.search_keys(q[:3], 10)),
             ("search_deep", lambda d: d.search_keys_deep(q, 2049)),
             ("search_filtered", lambda d: d.search_keys_filtered(q[:7], 100, member, q_set)),
             ("rank_rows", lambda d: d.rank_rows(q[:20], t_ptr, t_row)),
             ("search", lambda d: d.search_keys(q[:3], 10))]
    want = [fr.cut(dr.topk_rows(K[:3], 10), 10), dr.topk_rows(K, 2049), fr.masked_topk(K[:7], member, q_set, 100),
            drr.ranks_from_keys(K[:20], t_ptr, t_row)]
    want.append(want[0])
    alone = []
    for name, call in calls[:4]:
        dix = _open(c["p"], "f32")
        try:
            alone.append(call(dix))
        finally:
            dix.close()
    alone.append(alone[0])
    dix = _open(c["p"], "f32")
    try:
        first = [call(dix) for name, call in calls]
        before = dix.stats()
        second = [call(dix) for name, call in calls]
        assert dix.stats() == before and before["device_allocs"] > 0
    finally:
        dix.close()
    for (name, _), w, a, r1, r2 in zip(calls, want, alone, first, second):
        for got in (a, r1, r2):
            assert len(got) == len(w), name
            for g, x in zip(got, w):
                assert g.dtype == x.dtype and g.shape == x.shape and (g == x).all(), name
    for a, b in zip(first[0], first[4]):
        assert a.tobytes() == b.tobytes()


def test_small_index_one_tile(m):
    """At most 4096 rows: one 4096-row tile (another instance of the kernel)."""
    c = case("f32")
    n = 1000
    member = c["member"][:, :n]
    q_set = (np.arange(NQ) % 3 + 4).astype(np.int32)                           # even, span, random
    dix = _open(c["p"][:n], "f32")
    try:
        for k in (10, 1024):
            compare(dix.search_keys_filtered(c["q"], k, member, q_set), fr.masked_topk(c["K"][:, :n], member, q_set, k))
        # a set and its complement partition the rows (both lists whole: 500 rows each at k = 1024)
        both = np.stack([member[4], ~member[4]])
        a = dix.search_keys_filtered(c["q"], 1024, both, np.zeros(NQ, np.int32))
        b = dix.search_keys_filtered(c["q"], 1024, both, np.ones(NQ, np.int32))
        assert (a[2] == 500).all() and (b[2] == 500).all()
        for i in range(NQ):
            assert sorted(a[0][i, :500].tolist() + b[0][i, :500].tolist()) == list(range(n))
    finally:
        dix.close()


@PREC
def test_refusals_in_their_order(m, precision):
    from mllm_sparse_retrieval_amd import _cabi

    c = case(precision)
    lib, ptr = _cabi.lib(), _cabi.ptr
    idx, key, cnt = np.zeros((2, 8), np.uint32), np.zeros((2, 8), np.uint32), np.zeros(2, np.int32)
    is_f32 = 1 if precision == "f32" else 0
    q_ok = np.ascontiguousarray(c["q"][:2]) if is_f32 else np.ascontiguousarray(c["q"][:2].astype(np.float16))
    bits = fr.pack(np.ones((3, 300), dtype=bool))                                  # three full sets over the 300 rows
    qs, bad_qs = np.array([2, -1], np.int32), np.array([3, 0], np.int32)
    dix = _open(c["p"][:300], precision)
    try:
        def call(f32=is_f32, k=8, n_sets=3, b=bits, s=qs, q=q_ok, nq=2, out=idx):
            return lib.msr_dense_search_filtered(dix._h, ptr(q), f32, nq, k, ptr(b), n_sets, ptr(s), ptr(out), ptr(key), ptr(cnt), None)
        err = lib.msr_last_error
        # 1. MSR_E_INVAL, each before any MSR_E_RANGE cause
        assert call(out=None) == INVAL and call(q=None) == INVAL and call(nq=-1) == INVAL
        assert call(n_sets=-1) == INVAL and call(b=None) == INVAL and b"set_bits" in err()
        assert call(s=None) == INVAL and b"q_set" in err()
        assert call(f32=1 - is_f32) == INVAL and b"q_is_f32" in err()
        assert call(f32=1 - is_f32, k=0) == INVAL and call(b=None, k=0) == INVAL and call(s=None, n_sets=70000) == INVAL
        assert call(f32=1 - is_f32, s=bad_qs) == INVAL
        # 2. MSR_E_RANGE: k, then the number of sets, then the q_set entries
        for k in (0, -1, _cabi.MSR_KMAX + 1):
            assert call(k=k) == RANGE and b"MSR_KMAX" in err()
            assert call(k=k, n_sets=70000) == RANGE and b"MSR_KMAX" in err()
            assert call(k=k, s=bad_qs) == RANGE and b"MSR_KMAX" in err()
        assert call(n_sets=65537) == RANGE and b"MSR_FILTER_MAX_SETS" in err()
        assert call(n_sets=65537, s=np.array([70000, 0], np.int32)) == RANGE and b"MSR_FILTER_MAX_SETS" in err()
        for v in ([3, 0], [0, -2]):
            assert call(s=np.array(v, np.int32)) == RANGE and b"q_set[" in err()
        assert call(n_sets=0, b=None, s=np.array([0, -1], np.int32)) == RANGE
        # valid calls
        assert call(nq=0, q=None) == 0                                          # nq == 0: no launch
        assert call() == 0 and cnt.tolist() == [8, 8]
        assert call(n_sets=0, b=None, s=None) == 0 and call(n_sets=1, s=None) == 0
    finally:
        dix.close()
