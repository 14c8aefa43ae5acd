"""score_tiles_walk (csrc/msr_walk.hpp): one workgroup per query walks the tiles of a small index and keeps the running
top-k in LDS — no per-tile lists, no merge launch. Planted corpora, 1 100 queries per batch.

Two references, both compared for EQUALITY (ordinals, u32 scores, f32 bits, hit counts, padding):
  * the C oracle (oracle/taat.py through tests/helpers.py),
  * the same queries through the staged two-launch path, reached by calls of fewer than kWalkMinQueries queries.
The route a search took is read from msr_batch_debug_stamps()[7] (searches of the batch that walked).

CPU: the per-tile table a handle builds at attach time is what score_tiles computes per workgroup, restated from the
index file; the routing constants restated here are the ones in the source text."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import accum_ref as ar
from tests import helpers

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mllm_sparse_retrieval_amd", "csrc")
WALK_MAX_TILES, WALK_MAX_K, WALK_MIN_QUERIES = 8, 64, 1024
NQ = 1100
KS = (1, 10, 64)
N_FILL = 70
TIE_DOCS = 600          # equal-scored docs in tile 1: more than the 512-key candidate buffer holds
W_TOP = 40000           # 65535 * 40000 = 2 621 400 000 lies in [2^31, 2^32)


@pytest.fixture(scope="module")
def m(built):
    import mllm_sparse_retrieval_amd as m

    return m


# ------------------------------------------------------------------------------------------------------ corpus
def corpus(tile_docs, n_docs, seed=0):
    """Terms by role (ids in `roles`):
        dense   in 60 % of every tile's docs: the only term of the dense head
        only0   40 docs of tile 0;  only_last   up to 30 docs of the last tile;  rare   3 docs in all (tile 0 and the last)
        tie     weight 7 on the docs at offsets 5 and 6 of every tile: equal scores in different tiles
        mass    weight 9 on TIE_DOCS docs of tile 1 (all of them when the tile is smaller), 3 docs of tile 0
        low     weight 1 on 100 docs of tile 0: fills the running top-k with keys below every `mass` doc
        top     weight 65535 on two docs of every tile, 65534 on a third
        r0..r7  up to 200 docs per tile, weights 1-255;  fill  N_FILL terms of 1-8 docs per tile"""
    rng = np.random.default_rng(4242 + seed)
    sizes = [min(tile_docs, n_docs - t * tile_docs) for t in range(-(-n_docs // tile_docs))]
    T = len(sizes)
    last0 = (T - 1) * tile_docs
    roles, counts, explicit, at = {}, {}, {}, 0

    def new(name):
        nonlocal at
        roles[name] = at
        at += 1
        return at - 1

    counts[new("dense")] = [max(1, int(0.6 * nd)) if nd > 1 else 1 for nd in sizes]
    counts[new("only0")] = [40] + [0] * (T - 1)
    counts[new("only_last")] = [0] * (T - 1) + [min(30, sizes[-1])]
    rare_rows = [11, 12] + [last0 + sizes[-1] - 1]
    explicit[new("rare")] = (rare_rows, [3, 2, 4])
    tie_rows = [t * tile_docs + o for t in range(T) for o in (5, 6) if o < sizes[t]]
    explicit[new("tie")] = (tie_rows, [7] * len(tie_rows))
    if T > 1:
        n_mass = min(TIE_DOCS, sizes[1])
        mass_rows = [20, 21, 22] + (tile_docs + np.sort(rng.choice(sizes[1], size=n_mass, replace=False))).tolist()
        explicit[new("mass")] = (mass_rows, [9] * len(mass_rows))
    explicit[new("low")] = (np.sort(rng.choice(np.arange(100, sizes[0]), size=100, replace=False)).tolist(), [1] * 100)
    top_rows, top_w = [], []
    for t in range(T):
        for j, w in enumerate((65535, 65535, 65534)):
            if 30 + j < sizes[t]:
                top_rows.append(t * tile_docs + 30 + j)
                top_w.append(w)
    explicit[new("top")] = (top_rows, top_w)
    for i in range(8):
        counts[new(f"r{i}")] = [min(int(c), nd) for c, nd in zip(rng.integers(50, 201, size=T), sizes)]
    roles["fill"] = list(range(at, at + N_FILL))
    for i in range(N_FILL):
        counts[at] = [min(int(c), nd) for c, nd in zip(rng.integers(1, 9, size=T), sizes)]
        at += 1
    p = ar.plant(tile_docs, n_docs, at, counts, explicit=explicit, seed=seed)
    p.update(roles=roles, sizes=sizes)
    return p


def queries(p, with_65=False, seed=0):
    """NQ queries: the named cases first, then seeded mixes of the corpus' terms -> (csr, {name: query index})."""
    r, rng = p["roles"], np.random.default_rng(99 + seed)
    fill = r["fill"]
    named = {
        "no terms": [],
        "dense head only": [(r["dense"], 3)],
        "absent from some tiles": [(r["only0"], 2), (r["only_last"], 5), (r["r0"], 1)],
        "fewer than k hits": [(r["rare"], 5)],
        "all hits in the last tile": [(r["only_last"], 4)],
        "ties across tiles": [(r["tie"], 7)],
        "top of the score range": [(r["top"], W_TOP)],
        "64 sparse terms": [(t, 1 + i % 5) for i, t in enumerate(fill[:64])],
        "dense and sparse": [(r["dense"], 2), (r["r1"], 3), (r["r2"], 1), (fill[3], 9)],
    }
    if "mass" in r:
        named["candidate overflow"] = [(r["low"], 1), (r["mass"], 2)]
        named["mass ties alone"] = [(r["mass"], 1)]
    if with_65:
        named["65 sparse terms"] = [(t, 1 + i % 3) for i, t in enumerate(fill[:65])]
    qs, where = list(named.values()), {n: i for i, n in enumerate(named)}
    pool = [r["dense"], r["only0"], r["only_last"], r["tie"], r["low"]] + [r[f"r{i}"] for i in range(8)] + fill
    while len(qs) < NQ:
        n = int(rng.integers(1, 16))
        qs.append([(int(t), int(rng.integers(1, 200))) for t in rng.choice(pool, size=n, replace=False)])
    return ar.csr(qs), where


def _equal(a, b):
    for x, y in zip(a[:3], b[:3]):
        assert (np.ascontiguousarray(x).view(np.uint32) == np.ascontiguousarray(y).view(np.uint32)).all()
    assert (a[3] == b[3]).all()


def _staged(ix, q, k):
    """The same queries through the two-launch path: calls of fewer than kWalkMinQueries queries."""
    qp, qt, qw = q
    parts = []
    for lo in range(0, NQ, NQ // 2):
        hi = min(NQ, lo + NQ // 2)
        assert hi - lo < WALK_MIN_QUERIES
        parts.append(ix.search_csr(qp[lo:hi + 1] - qp[lo], qt[qp[lo]:qp[hi]], qw[qp[lo]:qp[hi]], k))
    return tuple(np.concatenate([x[i] for x in parts]) for i in range(4))


# (name, tile_docs, docs, walks?)
SHAPES = [("2 tiles, one doc in the last", 8192, 8193, True), ("3 full tiles", 8192, 3 * 8192, True),
          ("8 tiles", 8192, 7 * 8192 + 777, True), ("2 tiles of 4096", 4096, 4096 + 1500, True),
          ("9 tiles", 8192, 8 * 8192 + 5, False), ("1 tile", 8192, 5000, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,tile_docs,n_docs,walks", SHAPES, ids=[s[0].replace(" ", "_").replace(",", "") for s in SHAPES])
def test_walk_equals_oracle_and_staged_path(m, tmp_path, name, tile_docs, n_docs, walks):
    p = corpus(tile_docs, n_docs)
    path = ar.build(m, tmp_path / "w.idx", p, 1, 0.55)
    oix, _ = helpers.taat_oracle(p["docs"], p["n_terms"], p["ids"])
    q, where = queries(p)
    q65, where65 = queries(p, with_65=True)
    # the facts the cases are named after
    cen = ar.census(path, q, 10)
    assert cen["batch"]["light"] and cen["batch"]["max_sparse"] == 64 and cen["ix"]["n_dense"] == 2
    assert cen["queries"][where["64 sparse terms"]]["n_sparse"] == 64
    assert cen["queries"][where["dense head only"]]["dense_only"]
    assert cen["queries"][where["no terms"]]["n_sparse"] == 0 and not cen["queries"][where["no terms"]]["pairs"]
    cen65 = ar.census(path, q65, 10)
    assert not cen65["batch"]["light"] and cen65["queries"][where65["65 sparse terms"]]["n_sparse"] == 65
    with m.SparseIndex(path, device=0) as ix:
        assert ix.n_tiles == len(p["sizes"])
        b, b65 = ix.batch(*q, 65), ix.batch(*q65, 65)
        try:
            n_walked = 0
            for k in KS + (65,):
                want = oix.search(*q, k, threads=8)
                if k == 10:
                    self_check(p, where, want)
                b.search(k)
                got = b.fetch()
                n_walked += int(walks and k <= WALK_MAX_K)
                assert int(b.debug_stamps()[7]) == n_walked, (name, k)       # the route
                helpers.assert_same_results(got, want, k)
                _equal(got, _staged(ix, q, k))
                # one query of 65 sparse terms sends the whole batch down the staged path
                b65.search(k)
                got65 = b65.fetch()
                assert int(b65.debug_stamps()[7]) == 0
                helpers.assert_same_results(got65, oix.search(*q65, k, threads=8), k)
            assert b.debug_stamps()[:7].sum() == 0
        finally:
            b.close()
            b65.close()


def self_check(p, where, want):
    """What the named cases reach at k = 10, from the oracle's result."""
    w_ord, w_sc, w_n = want
    T, td = len(p["sizes"]), p["tile_docs"]
    assert w_n[where["no terms"]] == 0
    assert w_n[where["fewer than k hits"]] == 3
    i = where["all hits in the last tile"]
    assert w_n[i] == min(10, 30, p["sizes"][-1]) and (w_ord[i, :w_n[i]] >= (T - 1) * td).all()
    i = where["ties across tiles"]
    assert len(np.unique(w_sc[i, :w_n[i]])) == 1 and (np.diff(w_ord[i, :w_n[i]]) > 0).all()
    if T > 1 and p["sizes"][1] > 6:
        assert len(np.unique(w_ord[i, :w_n[i]] // td)) > 1                    # equal scores in different tiles
    i = where["top of the score range"]
    assert (w_sc[i, :w_n[i]] >= 2**31).all() and (w_sc[i, :w_n[i]] < 2**32).all()
    if "candidate overflow" in where and p["sizes"][1] >= TIE_DOCS:
        i = where["candidate overflow"]
        # tile 0 fills the top-10 (3 mass docs, then `low` docs); all TIE_DOCS mass docs of tile 1 beat its 10th key
        assert w_n[i] == 10 and (w_ord[i, :3] < td).all() and (w_ord[i, 3:] >= td).all() and (w_ord[i, 3:] < 2 * td).all()
        assert len(np.unique(w_sc[i])) == 1


# ------------------------------------------------------------------------------------------------------ CPU
def _lib():
    from mllm_sparse_retrieval_amd import _cabi

    lib = ctypes.CDLL(_cabi.LIB_PATH)
    lib.walk_tile_table.restype = ctypes.c_int
    lib.walk_tile_table.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    return lib


@pytest.mark.parametrize("tile_docs,n_docs", [(8192, 8193), (8192, 2 * 8192 + 2049), (4096, 7 * 4096 + 1024), (4096, 8192)])
def test_tile_table_is_what_score_tiles_computes(m, tmp_path, tile_docs, n_docs):
    p = corpus(tile_docs, n_docs)
    path = ar.build(m, tmp_path / "w.idx", p, 1, 0.55)
    f = helpers.read_index_file(path)
    nt = ar.INSTANCES[tile_docs][0]
    out = np.zeros((f["n_tiles"], 8), dtype=np.uint32)
    with m.SparseIndex(path, device=-1) as ix:
        assert _lib().walk_tile_table(ix._h, out.ctypes.data) == 0
    u64 = out.view(np.uint64)                                       # [n_tiles, 4]: seg_row, post_base, dense, (words 6, 7)
    for t in range(f["n_tiles"]):
        ndocs = min(tile_docs, n_docs - t * tile_docs)
        assert u64[t, 0] == t * (f["n_terms"] + 1) * 4              # seg_ptr + tile_l * (n_terms + 1)
        assert out[t, 6] == f["seg_ptr"][t, 0]                      # tile_first = seg_row[0]
        assert u64[t, 1] == (int(f["seg_ptr"][t, 0]) - int(f["seg_ptr"][0, 0])) * 16   # (tile_first - vec_base) * 16
        assert u64[t, 2] == t * (f["n_dense"] // 2) * tile_docs * 4  # dense + tile_l * n_pairs * TILE_DOCS * 4
        assert out[t, 7] & ~np.uint32(7) == t * tile_docs           # doc0
        assert out[t, 7] & 7 == -(-ndocs // (4 * nt))               # rounds
        assert 1 <= (out[t, 7] & 7) <= tile_docs // (4 * nt)


@pytest.mark.parametrize("tile_docs,n_docs", [(8192, 5000), (8192, 8 * 8192 + 1), (16384, 3 * 16384)])
def test_no_tile_table_outside_the_walk(m, tmp_path, tile_docs, n_docs):
    """One tile, more than kWalkMaxTiles tiles, a tile size without a light scorer: the handle never walks."""
    p = ar.plant(tile_docs, n_docs, 2, {0: [1] * (-(-n_docs // tile_docs))})
    path = ar.build(m, tmp_path / "w.idx", p)
    out = np.zeros((16, 8), dtype=np.uint32)
    with m.SparseIndex(path, device=-1) as ix:
        assert _lib().walk_tile_table(ix._h, out.ctypes.data) != 0
    assert not out.any()


def test_routing_constants_are_the_source_text():
    def src(name):
        with open(os.path.join(CSRC, name), encoding="utf-8") as f:
            return f.read()

    internal, dev, walk = src("msr_device_internal.hpp"), src("msr_device.hip"), src("msr_walk.hpp")
    assert re.search(rf"constexpr uint32_t kWalkMaxTiles = {WALK_MAX_TILES};", internal)
    assert re.search(rf"constexpr uint32_t kWalkMaxK = {WALK_MAX_K};", internal)
    assert re.search(rf"constexpr uint32_t kWalkMinQueries = {WALK_MIN_QUERIES};", internal)
    assert "return has_table && light_batch && !list_as_set && k <= kWalkMaxK && nq >= kWalkMinQueries;" in internal
    assert "walk_route(d->d_walk != nullptr, sa.light != 0, b->unsorted_ok, (uint32_t)b->nq, (uint32_t)k)" in dev
    assert "sa.light = b->max_sparse_terms <= 64 ? 1u : 0u;" in dev and ar.LIGHT_MAX == 64
    launcher = dev[dev.index("static int launch_walk("):dev.index("int launch_select(")]
    assert "a.n_tiles < 2 || a.n_tiles > kWalkMaxTiles || a.m.k > kWalkMaxK || !a.s.light || !a.tiles" in launcher
    assert "if constexpr (S::light)" in launcher and ar.LIGHT_TILES == (4096, 8192)
    wanted = dev[dev.index("static bool walk_table_wanted("):dev.index('extern "C" int walk_tile_table(')]
    assert "ix->term_nshards == 0 && hybrid_tile(h->tile_docs) && ix->shard_ntiles >= 2 && ix->shard_ntiles <= kWalkMaxTiles" in wanted
    assert "__shared__ uint64_t best[kWalkMaxK], side[kWalkMaxK];" in walk
