"""msr_hybrid_deep_filtered (dense.hybrid_deep_filtered) on the GPU, bit for bit: against tests/hybrid_filter_ref.fuse (the
sub-corpus reference, identity (b)) with every standard set spread over the queries of one call; against msr_hybrid_deep
(identity (a)), msr_search_filtered and msr_search_deep (identity (c)); after calls that leave other scores in the scratch;
on planted set boundaries; many alphas against single calls; a call of two passes whose sets differ between the passes; the
steady state of the scratch; the refusals with their codes and order; the command end to end. Every assertion on the call
is an equality. The corpora are those of tests/test_hybrid_deep.py."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import fusion_ref as fr
from tests import hybrid_filter_ref as hf
from tests import rank_ref
from tests.f32_chain import f32_keys
from tests.test_fuse_rows_ref import DEPTH, N_DEEP
from tests.test_hybrid_deep import K_EDGES, _bits, _case, _check_lists, _check_slice, _Handles, _k_max, _same

pytestmark = pytest.mark.gpu

E_INVAL, E_NODEVICE, E_RANGE = -1, -5, -8
DEPTHS = (1, 100, DEPTH, N_DEEP)
ALPHAS = (0.0, 1.0, 0.5, -0.25, 1.5)
FIELDS = ("ords", "scores", "n", "members", "src", "sparse_ords", "sparse_u32", "sparse_n", "dense_ords", "dense", "dense_n",
          "score_range")


@pytest.fixture(scope="module")
def m(built):
    import mllm_sparse_retrieval_amd as m

    return m


@pytest.fixture(scope="module")
def paths(m, tmp_path_factory):
    """Index files, built once per module: (case name, tile_docs) -> path."""
    root = tmp_path_factory.mktemp("hybrid_filtered")
    out = {}
    for name, tile in (("planted", 4096), ("planted", 12288), ("exact", 4096), ("floats", 4096), ("small", 4096)):
        case = _case(name)[0]
        ids = ["%07d" % o for o in case["r2o"]]
        out[name, tile] = m.build_index_from_csr(str(root / f"{name}_{tile}.idx"), *rank_ref.docs_to_csr(case["Dm"]),
                                                 case["Dm"].shape[1], doc_ids=ids, tile_docs=tile)
    return out


class _Filtered(_Handles):
    def filt(self, depth, k, alphas, sets, q_set, with_lists=True, self_ord="case"):
        from mllm_sparse_retrieval_amd.dense import hybrid_deep_filtered

        so = self.case["self_ord"] if isinstance(self_ord, str) else self_ord
        return hybrid_deep_filtered(self.ix, self.dix, *self.csr, self.case["q"], depth, k, alphas, self.case["r2o"], sets, q_set,
                                    so, with_lists=with_lists)


def _sets(name):
    return hf.standard_sets(_case(name)[1].shape[1], DEPTH)


def _rot(nq, r):
    """Every standard set and -1 spread over the queries of one call: query i takes entry (i + r) mod 9 of (-1, 0, .., 7)."""
    return ((np.arange(nq) + r) % 9 - 1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _ref(name, depth, alpha, r):
    case, S, D = _case(name)
    return hf.fuse(S, D, _sets(name), _rot(len(S), r), depth, alpha, case["self_ord"])


def _same_result(got, want, what, rows=slice(None)):
    for f in FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        if f in ("ords", "scores", "n", "src"):
            a, b = a[:, rows], b[:, rows]
        else:
            a, b = a[rows], b[rows]
        _same(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b, what + (f,))


# ------------------------------------------------------------------------------------------ b. the sub-corpus reference
@pytest.mark.parametrize("name,tile,prec", [("planted", 4096, "f32"), ("planted", 4096, "fp16"), ("planted", 12288, "fp16"),
                                            ("exact", 4096, "f32"), ("exact", 4096, "fp16"), ("floats", 4096, "f32"),
                                            ("small", 4096, "f32"), ("small", 4096, "fp16")])
def test_every_set_in_one_call_against_the_reference(m, paths, name, tile, prec):
    """full, empty, the single last doc, only the ragged third tile, ordinals < DEPTH and < DEPTH + 1 (exactly depth and
    depth + 1 members at depth DEPTH), a random half, a random tenth and -1 over the queries of ONE call, rotated so that
    every query meets several of them; all k edges on the planted f32 handle, the whole union elsewhere."""
    sets = _sets(name)
    with _Filtered(m, paths, name, tile, prec) as hd:
        nq = len(hd.case["queries"])
        for j, depth in enumerate(DEPTHS):
            rots = (j, j + 4, j + 7) if (name, prec) == ("planted", "f32") else (2 * j + 1,)
            for r in rots:
                want = _ref(name, depth, 0.3, r)
                ks = {_k_max(depth)}
                if (name, prec, r) == ("planted", "f32", j):
                    ks |= {1} | {k for k in K_EDGES if k <= _k_max(depth)}
                for k in sorted(ks):
                    res = hd.filt(depth, k, [0.3], sets, _rot(nq, r))
                    what = (name, tile, prec, depth, k, r)
                    _check_slice(res, 0, want, k, what)
                    _check_lists(res, want, depth, what)
                    assert res.ms["passes"] == 1 and res.ms["mask"] > 0
    if name == "planted":                                        # the reference holds what the sets promise
        want, q_set = _ref(name, DEPTH, 0.3, 2), _rot(8, 2).tolist()
        assert want.cnt[q_set.index(1)] == 0 and (want.rng[q_set.index(1)] == 0).all()            # (d) the empty set
        assert len(want.d_lists[q_set.index(4)][0]) == DEPTH == len(want.d_lists[q_set.index(5)][0])
        assert len(want.d_lists[q_set.index(2)][0]) == 1 and len(want.d_lists[q_set.index(3)][0]) == N_DEEP - 8192


# ------------------------------------------------------------------------------------------ a. the unfiltered call
@pytest.mark.parametrize("name,tile,prec", [("planted", 4096, "fp16"), ("planted", 12288, "f32"), ("small", 4096, "fp16")])
def test_full_set_unfiltered_and_no_set_are_hybrid_deep(m, paths, name, tile, prec):
    sets = _sets(name)
    with _Filtered(m, paths, name, tile, prec) as hd:
        nq = len(hd.case["queries"])
        for depth, k in ((100, 200), (DEPTH, _k_max(DEPTH))):
            base = hd.deep(depth, k, [0.3, 1.5])
            for what, s, q_set in (("full", sets, np.zeros(nq, np.int32)), ("-1", sets, np.full(nq, -1, np.int32)),
                                   ("one full set, no q_set", sets[:1], None), ("no set", sets[:0], None)):
                res = hd.filt(depth, k, [0.3, 1.5], s, q_set)
                _same_result(res, base, (name, prec, depth, what))
                assert (res.ms["mask"] > 0) == (what in ("full", "one full set, no q_set"))
            # a mixed call: the unfiltered queries and those of the full set are rows of hybrid_deep, whatever the others take
            q_set = _rot(nq, 0)
            res = hd.filt(depth, k, [0.3, 1.5], sets, q_set)
            _same_result(res, base, (name, prec, depth, "mixed"), rows=np.flatnonzero(q_set <= 0))
            assert not (res.members[q_set > 0] == base.members[q_set > 0]).all()


# ------------------------------------------------------------------------------------------ c. the sparse routes
def test_sparse_list_is_the_filtered_search_and_the_struck_deep_search(m, paths):
    sets = _sets("exact")
    with _Filtered(m, paths, "exact", 4096, "f32") as hd:
        nq = len(hd.case["queries"])
        q_set = _rot(nq, 3)
        res = hd.filt(1000, 1, [0.5], sets, q_set)
        o, _, u, n = hd.ix.search_filtered(*hd.csr, 1000, sets, q_set)
        _same(res.sparse_n, n, ("filtered n",))
        _same(res.sparse_ords, o, ("filtered ordinals",))
        _same(res.sparse_u32, u, ("filtered scores",))
        res = hd.filt(DEPTH, 1, [0.5], sets, q_set)
        o, _, u, n = hd.ix.search_deep(*hd.csr, N_DEEP)            # every hit, then the non-members struck out and the cut
        assert n.max() > 0
        for i in range(nq):
            keep = np.ones(n[i], bool) if q_set[i] < 0 else sets[q_set[i]][o[i, :n[i]]]
            wo, wu = o[i, :n[i]][keep][:DEPTH], u[i, :n[i]][keep][:DEPTH]
            assert res.sparse_n[i] == len(wo), i
            _same(res.sparse_ords[i, :len(wo)], wo, ("struck ordinals", i))
            _same(res.sparse_u32[i, :len(wo)], wu, ("struck scores", i))
            assert (res.sparse_ords[i, len(wo):] == fr.PAD).all() and (res.sparse_u32[i, len(wo):] == 0).all()


# ------------------------------------------------------------------------------------------ stale scratch
@pytest.mark.parametrize("tile", [4096, 12288])
def test_skipped_segments_hold_no_scores_of_an_earlier_call(m, paths, tile):
    """One pair of handles: an unfiltered call fills both score rows, then every query takes a set without a doc in tiles 0
    and 1 (4096-doc tiles: their dump segments are skipped) and then the empty set (every segment is skipped)."""
    sets = _sets("planted")
    case, S, D = _case("planted")
    with _Filtered(m, paths, "planted", tile, "fp16") as hd:
        k = _k_max(DEPTH)
        hd.deep(DEPTH, k, [0.3])
        for s in (3, 1, 2):
            q_set = np.full(8, s, np.int32)
            want = hf.fuse(S, D, sets, q_set, DEPTH, 0.3, case["self_ord"])
            res = hd.filt(DEPTH, k, [0.3], sets, q_set)
            _check_slice(res, 0, want, k, ("stale", tile, s))
            _check_lists(res, want, DEPTH, ("stale", tile, s))
            if s == 1:                                           # (d): nothing anywhere
                assert (res.n == 0).all() and (res.members == 0).all() and (res.score_range == 0).all()
                assert (res.sparse_n == 0).all() and (res.dense_n == 0).all() and (res.ords == fr.PAD).all()
                assert (_bits(res.scores) == 0).all() and (res.src == 0).all() and (res.dense_ords == fr.PAD).all()
            hd.deep(DEPTH, k, [0.3])


# ------------------------------------------------------------------------------------------ planted set boundaries
@functools.lru_cache(maxsize=None)
def _boundary_sets():
    """Per-query sets over the planted corpus and the depth of the call, each with the property it is named for asserted."""
    case, S, D = _case("planted")
    n, so, depth = N_DEEP, case["self_ord"], 400
    o = np.arange(n)
    sets = np.ones((8, n), bool)
    base = fr.fuse(S, D, depth, 0.3, so)
    # 0: cuts the dense tie class of the boundary: every other doc of the class is no member, and the boundary of the
    #    filtered list still falls inside the class (members and non-members share the boundary key)
    key = f32_keys(D[0] + fr.F0).astype(np.int64)
    order = np.lexsort((o, -key))
    cls = order[key[order] == key[order[depth - 1]]]
    sets[0, cls[::2]] = False
    above = int((key > key[cls[0]]).sum())
    assert above < depth < above + len(cls[1::2]) and len(cls) > 8
    # 1: excludes the query's best sparse docs and its best dense docs (each a tie class): both maxima move
    sets[1] = (S[1] < S[1].max()) & (D[1] < D[1].max())
    assert not sets[1, base.s_lists[1][0][0]] and not sets[1, base.d_lists[1][0][0]]
    # 2: fewer sparse hits than depth among more members than depth
    hits = np.flatnonzero(S[2] > 0)
    sets[2] = False
    sets[2, hits[:depth - 30]] = True
    sets[2, np.flatnonzero(S[2] == 0)[:depth + 30]] = True
    # 3, 4: self_ord (the best / the last of the unfiltered dense list) inside a small set, 5, 6: outside it
    for i in (3, 4, 5, 6):
        sets[i] = (o % 3 == 0) | (o == so[i]) if i < 5 else (o % 3 == 0) & (o != so[i])
    # 7: exactly depth - 1 members (query 7: no sparse hit, an all-zero dense row)
    sets[7] = o < depth - 1
    sets.setflags(write=False)
    return sets, depth


def test_planted_set_boundaries(m, paths):
    case, S, D = _case("planted")
    sets, depth = _boundary_sets()
    q_set = np.arange(8, dtype=np.int32)
    want = hf.fuse(S, D, sets, q_set, depth, 0.3, case["self_ord"])
    unf = fr.fuse(S, D, depth, 0.3, case["self_ord"])
    # the reference shows what the sets plant
    d0 = want.d_lists[0]
    nxt = np.flatnonzero(sets[0] & (D[0] == d0[1][-1]) & (np.arange(N_DEEP) > d0[0][-1]))
    assert len(nxt) > 0 and (~sets[0] & (D[0] == d0[1][-1])).any()          # the boundary key: members beyond it, non-members
    assert want.rng[1, 0] < unf.rng[1, 0] and want.rng[1, 2] < unf.rng[1, 2]   # both maxima moved
    assert len(want.s_lists[2][0]) == depth - 30 and len(want.d_lists[2][0]) == depth
    assert all(case["self_ord"][i] in want.d_lists[i][0] for i in (3,)) and want.cnt[7] == depth - 1
    for prec in ("f32", "fp16"):
        with _Filtered(m, paths, "planted", 4096, prec) as hd:
            for k in (1, 2 * depth):
                res = hd.filt(depth, k, [0.3], sets, q_set)
                _check_slice(res, 0, want, k, ("boundaries", prec, k))
                _check_lists(res, want, depth, ("boundaries", prec, k))
            # exactly depth, depth - 1 and depth + 1 members, with and without self_ord among them
            o = np.arange(N_DEEP)
            three = np.stack([o < depth, o < depth - 1, o < depth + 1])
            for so in (None, np.array([5, 5, 5, depth - 2, depth - 1, depth, depth + 1, -1], np.int32)):
                qs = np.array([0, 1, 2, 0, 1, 2, 0, 1], np.int32)
                w3 = hf.fuse(S, D, three, qs, depth, 0.3, so)
                res = hd.filt(depth, 2 * depth, [0.3], three, qs, self_ord=so)
                _check_slice(res, 0, w3, 2 * depth, ("members", prec))
                _check_lists(res, w3, depth, ("members", prec))
                assert res.dense_n.tolist() == [depth, depth - 1, depth, depth, depth - 1, depth, depth, depth - 1]


# ------------------------------------------------------------------------------------------ alphas
def test_five_alphas_against_single_calls_in_any_order(m, paths):
    sets = _sets("planted")
    q_set = _rot(8, 5)
    with _Filtered(m, paths, "planted", 12288, "f32") as hd:
        k = 2 * DEPTH
        res = hd.filt(DEPTH, k, ALPHAS, sets, q_set)
        assert res.ords.shape == res.scores.shape == res.src.shape == (5, 8, k) and res.n.shape == (5, 8)
        neg = False
        for a, alpha in enumerate(ALPHAS):
            _check_slice(res, a, _ref("planted", DEPTH, alpha, 5), k, ("sweep", alpha))
            one = hd.filt(DEPTH, k, [alpha], sets, q_set)
            for x, y in ((one.ords[0], res.ords[a]), (_bits(one.scores[0]), _bits(res.scores[a])), (one.n[0], res.n[a]),
                         (one.src[0], res.src[a]), (one.members, res.members)):
                _same(x, y, ("single call", alpha))
            neg = neg or bool((_bits(res.scores[a]) >> 31).any())
        assert neg
        _check_lists(res, _ref("planted", DEPTH, 0.0, 5), DEPTH, ("sweep",))
        perm = [3, 0, 4, 2, 1]
        rev = hd.filt(DEPTH, k, [ALPHAS[i] for i in perm] + [0.3], sets, q_set)
        for j, i in enumerate(perm):
            _same(rev.ords[j], res.ords[i], ("order", i))
            _same(_bits(rev.scores[j]), _bits(res.scores[i]), ("order", i))
            _same(rev.src[j], res.src[i], ("order", i))
        # (e) the sets of the other queries: query 0 alone in its set, every other query moved to another one
        other = q_set.copy()
        other[1:] = (other[1:] + 3) % 9 - 1
        assert other[0] == q_set[0] and (other[1:] != q_set[1:]).all()
        _same_result(hd.filt(DEPTH, k, [0.5], sets, other), hd.filt(DEPTH, k, [0.5], sets, q_set), ("other queries' sets",),
                     rows=slice(0, 1))


# ------------------------------------------------------------------------------------------ passes, scratch
def test_a_call_of_two_passes_with_sets_that_differ_between_them(m, paths):
    """5 400 queries over rows of 12 288 columns take two passes (5 376 + 24). The queries are the case's eight, repeated;
    repetition r takes rotation r mod 9 of the sets, so the second pass (repetition 672 onward: rotation 6) uses other sets
    than the first rows of the first pass: q_set indexed by the pass's row instead of the call's query shows."""
    from mllm_sparse_retrieval_amd.dense import hybrid_deep_filtered

    reps, depth, k = 675, 100, 10
    sets = _sets("planted")
    with _Filtered(m, paths, "planted", 12288, "fp16") as hd:
        case = hd.case
        ones = [hd.filt(depth, k, [0.3, 1.5], sets, _rot(8, r)) for r in range(9)]
        q_set = np.concatenate([_rot(8, r % 9) for r in range(reps)])
        big = hybrid_deep_filtered(hd.ix, hd.dix, *rank_ref.csr(case["queries"] * reps), np.tile(case["q"], (reps, 1)), depth,
                                   k, [0.3, 1.5], case["r2o"], sets, q_set, np.tile(case["self_ord"], reps))
        assert big.ms["passes"] == 2 and ones[0].ms["passes"] == 1 and (5376 // 8) % 9 != 0
        for f in FIELDS:
            got = getattr(big, f)
            per_alpha = f in ("ords", "scores", "n", "src")
            want = np.concatenate([getattr(ones[r % 9], f) for r in range(reps)], axis=1 if per_alpha else 0)
            _same(got.view(np.uint32) if got.dtype == np.float32 else got,
                  want.view(np.uint32) if want.dtype == np.float32 else want, (f,))


def test_a_repeated_call_allocates_nothing(m, paths):
    sets = _sets("exact")
    with _Filtered(m, paths, "exact", 4096, "fp16") as hd:
        q_set = _rot(8, 1)
        first = hd.filt(2000, 4000, [0.3, 0.6], sets, q_set)
        before = hd.dix.stats()
        again = hd.filt(2000, 4000, [0.3, 0.6], sets, q_set)
        smaller = hd.filt(500, 100, [0.1], sets[:2], np.zeros(8, np.int32), with_lists=False)
        plain = hd.deep(2000, 4000, [0.3, 0.6])
        assert hd.dix.stats() == before and before["device_allocs"] > 0
        _same(again.ords, first.ords, ("repeat",))
        _same(_bits(again.scores), _bits(first.scores), ("repeat",))
        assert smaller.n.shape == (1, 8) and smaller.src is None and plain.n.shape == (2, 8)


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_and_their_order(m, paths):
    from mllm_sparse_retrieval_amd import _cabi
    from mllm_sparse_retrieval_amd.dense import DenseIndex
    from mllm_sparse_retrieval_amd.filters import pack_doc_sets

    L = _cabi.lib()
    case = _case("small")[0]
    qp, qt, qw = _cabi.as_csr(*rank_ref.csr(case["queries"]))
    nq = len(qp) - 1
    q32 = np.ascontiguousarray(case["q"], dtype=np.float32)
    r2o = np.ascontiguousarray(case["r2o"], dtype=np.uint32)
    o, f = np.zeros((2, nq, 8), np.uint32), np.zeros((2, nq, 8), np.float32)
    n, mem = np.zeros((2, nq), np.int32), np.zeros(nq, np.uint32)
    bits2 = pack_doc_sets(_sets("small")[[0, 6]])
    qs_ok = np.zeros(nq, np.int32)
    ms = (ctypes.c_float * 7)()
    p = _cabi.ptr

    def call(ix, dx, depth=4, k=8, alphas=(0.5,), n_alphas=None, is_f32=1, nq_=nq, q=q32, out=o, bits=bits2, n_sets=2,
             q_set=qs_ok):
        al = np.asarray(alphas, dtype=np.float32)
        rc = L.msr_hybrid_deep_filtered(ix, dx, p(qp), p(qt), p(qw), p(q), is_f32, nq_, depth, k, p(al),
                                        len(al) if n_alphas is None else n_alphas, 0, p(r2o), None, p(bits), n_sets, p(q_set),
                                        p(out), p(f), p(n), p(mem), None, None, None, None, None, None, None, None, ms)
        return rc, L.msr_last_error().decode()

    bad_qs = qs_ok.copy()
    bad_qs[-1] = 2
    dix = DenseIndex(case["p"], precision="f32")
    other = DenseIndex(case["p"][:100], precision="f32")
    try:
        with m.SparseIndex(paths["small", 4096], device=-1) as host, m.SparseIndex(paths["small", 4096], device=0) as ix:
            # everything wrong at once on a handle without a device: MSR_E_INVAL first, the sets' shapes included ...
            for kw in (dict(out=None), dict(nq_=-1), dict(q=None), dict(is_f32=0), dict(alphas=(0.5, float("nan"))),
                       dict(n_sets=-1), dict(bits=None), dict(q_set=None)):
                rc, msg = call(host._h, dix._h, depth=0, k=0, **dict(dict(q_set=bad_qs), **kw))
                assert rc == E_INVAL and "msr_hybrid_deep_filtered" in msg, (kw, msg)
            rc, msg = call(host._h, other._h, depth=0)
            assert rc == E_INVAL and "100 rows" in msg
            # ... then MSR_E_RANGE: depth, k, n_alphas before the sets' ranges ...
            for kw, word in ((dict(depth=0), "depth"), (dict(depth=16385), "depth"), (dict(k=0), "k must"), (dict(k=9), "k must"),
                             (dict(depth=16384, k=16385), "k must"), (dict(n_alphas=0), "n_alphas"),
                             (dict(alphas=(0.5,) * 65), "n_alphas")):
                rc, msg = call(host._h, dix._h, q_set=bad_qs, **kw)
                assert rc == E_RANGE and word in msg and "msr_hybrid_deep_filtered" in msg, (kw, msg)
            for kw, word in ((dict(q_set=bad_qs), "q_set"), (dict(q_set=np.full(nq, -2, np.int32)), "q_set"),
                             (dict(n_sets=65537), "MSR_FILTER_MAX_SETS")):
                rc, msg = call(host._h, dix._h, **kw)
                assert rc == E_RANGE and word in msg and "msr_hybrid_deep_filtered" in msg, (kw, msg)
            # ... then MSR_E_NODEVICE
            rc, msg = call(host._h, dix._h)
            assert rc == E_NODEVICE
            # nq == 0 is MSR_OK; well-formed calls, q_set = NULL with one set and with none
            assert call(ix._h, dix._h, nq_=0)[0] == 0
            assert call(ix._h, dix._h)[0] == 0
            assert call(ix._h, dix._h, n_sets=1, q_set=None)[0] == 0
            assert call(ix._h, dix._h, bits=None, n_sets=0, q_set=None)[0] == 0
            # a precision mismatch on a device handle
            rc, msg = call(ix._h, dix._h, is_f32=0)
            assert rc == E_INVAL and "msr_hybrid_deep_filtered" in msg
    finally:
        dix.close()
        other.close()
    with m.SparseIndex(paths["planted", 4096], device=0, shard=0, n_shards=2) as sh:
        dix = DenseIndex(_case("planted")[0]["p"], precision="f32")
        try:
            wide = pack_doc_sets(_sets("planted")[[0, 6]])
            rc, msg = call(sh._h, dix._h, bits=wide)
            assert rc == E_INVAL and "shard" in msg and "msr_hybrid_deep_filtered" in msg
        finally:
            dix.close()


# ------------------------------------------------------------------------------------------ the command, end to end
def test_cli_fusion_filtered_against_host_fusion(m, tmp_path_factory):
    """search --fusion_filtered with five fold sets (every 7th query unfiltered, one doc in no set: the corpus of
    tests/test_cli_filtered.py at dense dimension 32, where the hybrid route and the dense search take the same fp16 GEMM
    instance) against --host_fusion --doc_sets at depth 100: sparse.trec line for line, the same docs per query in
    dense.trec and fusion.trec, fused scores within 1e-5 (the bound tests/test_hybrid_deep.py holds GPU-fused f32 scores to
    against fuse() in Python doubles). Tie orders between the two may differ: sets and scores."""
    from mllm_sparse_retrieval_amd import cli
    from mllm_sparse_retrieval_amd.cli import _index_path, read_queries
    from mllm_sparse_retrieval_amd.fusion import read_trec_run

    root = tmp_path_factory.mktemp("cli_fusion_filtered")
    enc, dense, queries = str(root / "enc"), str(root / "dense"), str(root / "queries.tsv")
    cli.main(["encode", "--synthetic", "flickr", "--n_images", "2000", "--sparse_output_dir", enc, "--threads", "4",
              "--dense_output_dir", dense, "--dense_dim", "32"])
    cli.main(["index", "--input", enc, "--threads", "4", "--impact", "--pretokenized"])
    with open(os.path.join(enc, "query.tsv")) as f, open(queries, "w") as g:
        g.writelines(f.readlines()[:300])
    qids, _ = read_queries(queries)
    with m.SparseIndex(_index_path(enc), device=-1) as meta:
        docids = meta.docid_table().tolist()
    fold_of_doc = {d: "fold%d" % (j % 5) for j, d in enumerate(docids) if j != 3}
    fold_of_q = {q: "fold%d" % (i % 5) for i, q in enumerate(qids) if i % 7 != 6}
    (root / "doc_sets.tsv").write_text("".join(f"{d}\t{s}\n" for d, s in fold_of_doc.items()))
    (root / "query_sets.tsv").write_text("".join(f"{q}\t{s}\n" for q, s in fold_of_q.items()))
    common = ["search", "--query_type", "text", "--dataset_name", "flickr", "--quiet", "--sparse_index", enc, "--passage_reps",
              dense, "--queries", queries, "--depth", "100", "--alpha", "0.3", "--doc_sets", str(root / "doc_sets.tsv"),
              "--query_sets", str(root / "query_sets.tsv")]
    cli.main(common + ["--save_dir", str(root / "gpu"), "--fusion_filtered", "--alphas", "0,0.3,1", "--sweep_runs"])
    cli.main(common + ["--save_dir", str(root / "host"), "--host_fusion"])
    with open(root / "gpu" / "sparse.trec") as f, open(root / "host" / "sparse.trec") as g:
        a, b = f.readlines(), g.readlines()
    assert len(a) == len(b) > 0 and a == b
    got, want = read_trec_run(str(root / "gpu" / "fusion.trec")), read_trec_run(str(root / "host" / "fusion.trec"))
    gd, wd = read_trec_run(str(root / "gpu" / "dense.trec")), read_trec_run(str(root / "host" / "dense.trec"))
    assert set(got) == set(want) == set(gd) == set(wd) and len(got) == 300
    worst = 0.0
    for qid in want:
        fold = fold_of_q.get(qid)
        assert all(fold is None or fold_of_doc.get(d) == fold for d in got[qid]["docs"]), qid
        assert set(gd[qid]["docs"]) == set(wd[qid]["docs"]) and len(gd[qid]["docs"]) == 100, qid
        assert set(got[qid]["docs"]) == set(want[qid]["docs"]), qid
        worst = max(worst, max(abs(got[qid]["docs"][d] - x) for d, x in want[qid]["docs"].items()))
    print("largest fused score difference:", worst)
    assert worst <= 1e-5
    assert any(q not in fold_of_q for q in got) and max(len(v["docs"]) for v in got.values()) > 100
    mid = read_trec_run(str(root / "gpu" / "fusion.alpha_0.3.trec"))
    assert {q: v["docs"] for q, v in mid.items()} == {q: v["docs"] for q, v in got.items()}
    assert all(os.path.exists(root / "gpu" / f"fusion.alpha_{x}.trec") for x in ("0", "1"))
