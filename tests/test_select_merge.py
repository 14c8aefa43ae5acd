"""The selection and merge kernels every search path shares, aimed at their branch edges and checked against exact
references built here (tests/select_ref.py): merge_small / merge_lists through msr_merge_lists, and select_tiles +
sparsify_keys through msr_sparsify.

Branches of the merge (csrc/msr_device.hip launch_merge, csrc/msr_kernels.hpp merge_lists):
    merge_small              n_lists * k <= 64 and k <= 64
    merge_lists "copy"       otherwise, n_lists == 1
    merge_lists "gather"     otherwise, n_lists * k <= kCandCap (1024)
    merge_lists "heads"      more keys than kCandCap, n_lists >= k: threshold = k-th largest list head
    merge_lists "bisect"     more keys than kCandCap and n_lists < k (or the head threshold keeps too many): 64-step
                             bisection over all keys
("more keys" counts the non-empty keys: lists whose keys all fit the buffer are gathered as they are.)"""
import numpy as np
import pytest

from tests.select_ref import log1p_relu_f16, log1p_relu_f32, merge_ref

pytestmark = pytest.mark.gpu

MODES = ("random", "one_score", "few_scores", "extremes", "empty", "short")


@pytest.fixture(scope="module")
def ix(built, tmp_path_factory):
    import mllm_sparse_retrieval_amd as m

    dp, dt, dw = m.synth_vectors(100, 8, 200, seed=5)
    path = m.build_index_from_csr(str(tmp_path_factory.mktemp("merge") / "h.idx"), dp, dt, dw, 200, tile_docs=4096)
    with m.SparseIndex(path, device=0) as h:  # any handle: msr_merge_lists only needs its device and stream
        yield h


def _lists(rng, n_lists, nq, k, modes):
    """Best-first host lists [n_lists, nq, k]; query q gets content modes[q % len(modes)]. Ordinals are distinct within
    a query (as tiles and shards partition the docs); slots past a list's count hold junk the merge must ignore."""
    ords = rng.integers(0, 2**32, size=(n_lists, nq, k), dtype=np.uint64).astype(np.uint32)
    sc = rng.integers(0, 2**32, size=(n_lists, nq, k), dtype=np.uint64).astype(np.uint32)
    n = np.zeros((n_lists, nq), dtype=np.int32)
    for q in range(nq):
        mode = modes[q % len(modes)]
        if mode == "empty":
            cnt = np.zeros(n_lists, dtype=np.int64)
        elif mode == "short":  # many empty lists, the others shorter than k
            cnt = np.where(rng.random(n_lists) < 0.5, 0, rng.integers(0, k + 1, size=n_lists))
        else:  # every list full
            cnt = np.full(n_lists, k, dtype=np.int64)
        tot = int(cnt.sum())
        # distinct ordinals of [0, 0xFFFFFFFE], always including both ends when there is room
        pool = np.unique(rng.integers(1, 0xFFFFFFFE, size=tot + 16, dtype=np.uint64))
        pool = rng.permutation(np.concatenate([np.array([0, 0xFFFFFFFE], dtype=np.uint64), pool])[:tot])
        assert len(pool) == tot
        if mode == "random":
            s = rng.integers(1, 2**32, size=tot, dtype=np.uint64)
        elif mode == "one_score":
            s = np.full(tot, 777, dtype=np.uint64)
        elif mode == "few_scores":  # ties straddle the k-th position across lists
            s = rng.choice(np.array([5, 6, 7], dtype=np.uint64), size=tot)
        else:  # extremes, empty, short: the top of the u32 range, and the bottom
            s = rng.choice(np.array([0xFFFFFFFF, 0xFFFFFFFE, 2**31, 1], dtype=np.uint64), size=tot)
        at = 0
        for l in range(n_lists):
            c = int(cnt[l])
            o, v = pool[at : at + c].astype(np.int64), s[at : at + c].astype(np.int64)
            at += c
            order = np.lexsort((o, -v))  # best first: score descending, ordinal ascending
            ords[l, q, :c] = o[order]
            sc[l, q, :c] = v[order]
            n[l, q] = c
    return ords, sc, n


def _check_merge(ix, n_lists, nq, k, seed, modes=MODES):
    rng = np.random.default_rng(seed)
    ords, sc, n = _lists(rng, n_lists, nq, k, modes)
    o, sf, su, on = ix.merge_lists(ords, sc, n, k)
    w_o, w_s, w_n = merge_ref(ords, sc, n, k)
    assert (on == w_n).all(), (n_lists, k, np.flatnonzero(on != w_n)[:8])
    bad = np.argwhere((o != w_o) | (su != w_s))
    assert bad.size == 0, f"n_lists={n_lists} k={k}: {len(bad)} slots differ, first {bad[0]}: " \
                          f"({o[tuple(bad[0])]:#x}, {su[tuple(bad[0])]:#x}) vs ({w_o[tuple(bad[0])]:#x}, {w_s[tuple(bad[0])]:#x})"
    assert (sf.view(np.uint32) == w_s.astype(np.float32).view(np.uint32)).all()  # float32(u32), padding 0.0
    # non-empty keys per query: what merge_lists compares with kCandCap to pick its branch
    cnt = np.minimum(np.maximum(n, 0), k)
    return np.array([sum(int((sc[l, q, : cnt[l, q]] != 0).sum()) for l in range(n_lists)) for q in range(nq)])


# (n_lists, k) -> the branch it selects (launch_merge: n_lists * k <= 64 and k <= 64 -> merge_small; merge_lists:
# n_lists == 1 -> copy, n_lists * k <= 1024 -> gather, else heads when n_lists >= k, bisect otherwise)
MERGE_CASES = [
    (64, 1, "merge_small: 64 items, k = 1"),
    (1, 64, "merge_small: one list of k = 64"),
    (2, 32, "merge_small: 64 items"),
    (1, 65, "merge_lists copy: k = 65 leaves merge_small"),
    (65, 1, "merge_lists gather: 65 items at k = 1"),
    (5, 13, "merge_lists gather: 65 items"),
    (2, 64, "merge_lists gather: k = 64, 128 items"),
    (2, 65, "merge_lists gather: k = 65, 130 items"),
    (16, 64, "merge_lists gather: exactly 1024 items"),
    (1, 1024, "merge_lists copy: k = 1024"),
    (41, 25, "merge_lists heads: 1025 items, n_lists >= k"),
    (25, 41, "merge_lists bisect: 1025 items, n_lists < k"),
    (300, 10, "merge_lists heads: 3000 items"),
    (1024, 1, "merge_lists gather: 1024 items at k = 1"),
    (1025, 1, "merge_lists heads: 1025 items at k = 1"),
    (8, 200, "merge_lists bisect: 1600 items, n_lists < k"),
    (3, 1024, "merge_lists bisect: k = 1024, 3072 items"),
]


@pytest.mark.parametrize("n_lists,k,branch", MERGE_CASES, ids=[f"{a}x{b}" for a, b, _ in MERGE_CASES])
def test_merge_lists_branches(ix, n_lists, k, branch):
    # nq = 13: merge_small packs four queries per workgroup, the last one partly; every content mode appears twice
    keys = _check_merge(ix, n_lists, 13, k, seed=n_lists * 7919 + k)
    # the inputs select the branch the case names
    assert (keys[[MODES.index("empty"), MODES.index("empty") + 6]] == 0).all()
    if "heads" in branch or "bisect" in branch:
        assert keys.max() > 1024 and (n_lists >= k) == ("heads" in branch)
    elif "merge_lists" in branch:
        assert (n_lists * k > 64 or k > 64) and ((n_lists == 1) == ("copy" in branch)) and n_lists * k <= 1024
    else:
        assert n_lists * k <= 64 and k <= 64


def test_merge_lists_full_lists_force_bisection(ix):
    # every score equal: up to 3 x 1024 keys exceed kCandCap, n_lists < k, and the bisection must end on the shared
    # score with exactly the 1024 lowest ordinals (merge_lists "bisect")
    assert _check_merge(ix, 3, 4, 1024, seed=1, modes=("one_score",)).min() > 1024
    # 2048 / 1100 full lists at k = 1 (merge_lists "heads"): the threshold is the top key itself, one survivor, even
    # where every score is equal and only the ordinal decides
    assert _check_merge(ix, 2048, 2, 1, seed=2, modes=("one_score", "extremes")).min() > 1024
    assert _check_merge(ix, 1100, 3, 1, seed=3, modes=("one_score", "random", "few_scores")).min() > 1024


def test_merge_lists_caches_nothing_between_shapes(ix):
    # alternate branches on one handle: every call builds its own device buffers
    for n_lists, k in [(2, 32), (16, 64), (3, 1024), (2, 32), (1, 65)]:
        _check_merge(ix, n_lists, 5, k, seed=n_lists + k)


# ------------------------------------------------------------------------------------------------ sparsifier
def _sparsify(x, k, fp16_math=None):
    from mllm_sparse_retrieval_amd.sparsify import sparsify_logits

    return sparsify_logits(x, k, fp16_math=fp16_math)


def _rank_by_x(x, k):
    """Expected ids when distinct x values map to distinct values of log(1 + relu(x)): x descending, id ascending;
    every x <= 0 ties at value 0."""
    xr = np.maximum(np.nan_to_num(x.astype(np.float64), nan=0.0), 0)
    ids = np.broadcast_to(np.arange(x.shape[1]), x.shape)
    return np.lexsort((ids, -xr), axis=1)[:, :k].astype(np.uint32)


def _check_f32_values(x, ids, vals, w, k):
    # device logf is not correctly rounded: near log(1570) it was measured up to 2.14 f32 ulps off, so the bound is
    # OpenCL's for logf, three ulps of the float64 log
    v64, ulp = log1p_relu_f32(x)
    ulp = 3 * ulp
    got = np.take_along_axis(v64, ids.astype(np.int64), axis=1)
    gu = np.take_along_axis(ulp, ids.astype(np.int64), axis=1)
    assert (np.abs(vals.astype(np.float64) - got) <= gu).all(), np.abs(vals - got).max()
    assert (w == np.rint(vals * np.float32(100)).astype(np.int32)).all()  # src/encode.py:75, bit for bit
    assert (np.diff(vals.astype(np.float64), axis=1) <= 0).all()
    for r in range(x.shape[0]):
        out = np.ones(x.shape[1], bool)
        out[ids[r].astype(np.int64)] = False
        # nothing left out beats the k-th value returned by more than that bound
        assert (v64[r][out] <= float(vals[r, -1]) + gu[r, -1]).all()
        # among equal values, ids ascending
        same = np.diff(vals[r]) == 0
        assert (np.diff(ids[r].astype(np.int64))[same] > 0).all()


# vocab -> select_tiles instance (msr_sparsify: tile 4096 up to 4096 entries, else 8192) and tile count
VOCABS = [4096, 4097, 8192, 8193, 3 * 8192 + 1]  # 1 tile of 4096; 1 ragged of 8192; 1 full; 2 and 4 tiles, last 1 entry


@pytest.mark.parametrize("vocab", VOCABS)
def test_sparsify_f32_shapes(built, vocab):
    # levels j / 16: neighbouring values of log(1 + x) lie >= 80 f32 ulps apart, so the exact rank by x is the rank
    # by value whatever the rounding of device logf; repeated levels make exact ties, and negatives tie at 0
    rng = np.random.default_rng(vocab)
    rows = 3
    x = (rng.integers(-2000, 24000, size=(rows, vocab)) / 16).astype(np.float32)
    x[1, ::3] = x[1, 0]  # row 1: a third of the row shares one value
    # the largest values sit in the last (ragged) tile and straddle its first entry
    tile = 4096 if vocab <= 4096 else 8192
    last0 = (vocab - 1) // tile * tile
    top = np.float32(24000 / 16) + np.arange(1100, dtype=np.float32)[::-1] / 16
    for r in (0, 2):
        at = np.arange(max(last0 - 600, 0), min(last0 + 500, vocab))
        x[r, at] = rng.permutation(top[: len(at)])
        x[r, -1] = top[0] + 1
    for k in (1, 64, 65, 512, 513, 1024):
        ids, vals, w = _sparsify(x, k)
        want = _rank_by_x(x, k)
        bad = np.argwhere(ids != want)
        assert bad.size == 0, f"vocab={vocab} k={k}: {len(bad)} ids differ, first at {bad[0]}"
        _check_f32_values(x, ids, vals, w, k)


def test_sparsify_exact_ties(built):
    # repeated x values: among equal x the lower ids are kept, in ascending order, whatever device logf rounds to
    rng = np.random.default_rng(3)
    levels = np.array([-1.0, 0.25, 1.5, 3.0, 7.0], dtype=np.float32)
    for vocab, k in [(5000, 700), (20000, 1024), (9000, 65), (300, 64)]:
        x = rng.choice(levels, size=(4, vocab)).astype(np.float32)
        for dtype in (np.float32, np.float16):
            ids, vals, w = _sparsify(x.astype(dtype), k)
            assert (ids == _rank_by_x(x, k)).all(), (vocab, k, dtype)
            assert (w == np.rint(vals * np.float32(100)).astype(np.int32)).all()


def test_sparsify_mass_ties_and_nan(built):
    vocab, k = 9000, 1024
    x = np.zeros((4, vocab), dtype=np.float32)
    x[0] = 2.5  # every entry equal
    x[1] = -1.0  # no positive entry: every value 0
    x[2] = -3.0
    x[2, 8000:] = np.nan  # NaN logits: fmaxf(NaN, 0) = 0, so NaN ranks like a non-positive logit
    x[2, 100:110] = 4.0
    x[3, :] = np.nan
    ids, vals, w = _sparsify(x, k)
    assert (ids[0] == np.arange(k)).all() and (ids[1] == np.arange(k)).all() and (ids[3] == np.arange(k)).all()
    assert (vals[1] == 0).all() and (w[1] == 0).all() and (vals[3] == 0).all() and (w[3] == 0).all()
    assert (ids[2, :10] == np.arange(100, 110)).all()
    assert (ids[2, 10:] == np.setdiff1d(np.arange(k + 10), np.arange(100, 110))[: k - 10]).all()
    assert not np.isnan(vals).any()
    ids16, vals16, _ = _sparsify(x.astype(np.float16), k)
    assert (ids16 == ids).all() and (vals16[[1, 3]] == 0).all()


def test_sparsify_fp16_math_exhaustive(built):
    # every positive finite half (0x0001 .. 0x7BFF) at 1024 distinct positives per row, the rest of the row negative;
    # values bit for bit against f16(log(f16(1 + x))) except where the float64 log lies within one f32 ulp of a half
    # rounding midpoint (the exemption list, computed below and kept small)
    bits = np.arange(0x0001, 0x7C00, dtype=np.uint16)
    xs = bits.view(np.float16)
    per = 1024
    rows = (len(xs) + per - 1) // per
    vocab = 1500
    x = np.full((rows, vocab), np.float16(-1.0), dtype=np.float16)
    rng = np.random.default_rng(16)
    slot = np.full((rows, per), -1, dtype=np.int64)
    for r in range(rows):
        chunk = xs[r * per : (r + 1) * per]
        pos = np.sort(rng.choice(vocab, size=len(chunk), replace=False))
        x[r, pos] = rng.permutation(chunk)
        slot[r, : len(chunk)] = pos
    ids, vals, w = _sparsify(x, per)
    want, near = log1p_relu_f16(x)
    assert near.sum() <= 40, int(near.sum())  # the exemption list
    ii = ids.astype(np.int64)
    got_want = np.take_along_axis(want, ii, axis=1).astype(np.float32)
    got_near = np.take_along_axis(near, ii, axis=1)
    # the entries returned with a value above 0 are exactly the positives whose half log is above 0 (the rest of the
    # row ties at 0 and is taken by id)
    for r in range(rows):
        pos = slot[r][slot[r] >= 0]
        assert set(ids[r][vals[r] > 0].tolist()) == set(pos[want[r, pos] > 0].tolist())
    ok = (vals.view(np.uint32) == got_want.view(np.uint32)) | got_near
    assert ok.all(), f"{int((~ok).sum())} values differ, first at {np.argwhere(~ok)[0]}"
    assert (w == np.rint(vals * np.float32(100)).astype(np.int32)).all()
    # ids: value descending, then id ascending
    for r in range(rows):
        same = np.diff(vals[r]) == 0
        assert (np.diff(ids[r].astype(np.int64))[same] > 0).all()
    print(f"fp16 exhaustive: {len(xs)} inputs, {int(near.sum())} exempt")


def test_sparsify_k_above_vocab_is_refused(built):
    from mllm_sparse_retrieval_amd._cabi import MsrError

    x = np.ones((2, 100), dtype=np.float32)
    with pytest.raises(MsrError) as e:
        _sparsify(x, 101)
    assert e.value.code == -8  # MSR_E_RANGE, like torch.topk's refusal
    ids, vals, w = _sparsify(x, 100)  # k == vocab is fine
    assert (ids == np.arange(100)).all()


def test_sparsify_more_rows_than_grid_y(built):
    # 65 537 rows: sparsify_keys slices its rows against kMaxGridY (65 535); the rows of the second slice must be
    # scored as themselves
    rows, vocab, k = 65537, 40, 5
    r = np.arange(rows)
    x = np.full((rows, vocab), -1.0, dtype=np.float32)
    x[r, r % vocab] = 1 + (r % 7)  # the winner moves with the row
    x[r, (r + 11) % vocab] = 0.5
    ids, vals, w = _sparsify(x, k)
    bad = np.argwhere(ids != _rank_by_x(x, k))
    assert bad.size == 0, f"{len(bad)} ids differ, first at {bad[0]}"
    _check_f32_values(x[65530:], ids[65530:], vals[65530:], w[65530:], k)
    v64, ulp = log1p_relu_f32(np.float32(1) + (r % 7).astype(np.float32))
    assert (np.abs(vals[:, 0].astype(np.float64) - v64) <= 3 * ulp).all()
    assert (w == np.rint(vals * np.float32(100)).astype(np.int32)).all()
