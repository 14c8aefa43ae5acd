"""score_tiles_walk's cross-tile pipeline (csrc/msr_walk.hpp): the segment lookup, the scan and the first UL chunk loads
per wave of tile t+1 are issued around tile t's "accumulation complete" barrier and held in registers across tile t's
selection. What that loop can get wrong and tests/test_walk.py does not reach:

  * chunk counts per wave that change from tile to tile (idle slots after busy ones and the reverse, the leftover loop
    — more than UL chunks per wave — in the same tile as a held prefetch),
  * every selection path while the next tile's postings are held: the full tile_select after an empty first tile, a
    theta_select that overflows its 512 keys (in a middle tile and in the last, where nothing is held), hits only in
    the last tile, queries without sparse terms or without terms,
  * 2 tiles with a one-doc last tile, and 8 tiles.

Planted corpora (tests/accum_ref.py), 1 100 queries per batch so that the batch walks (msr_batch_debug_stamps()[7]),
named cases first. Both references are compared for EQUALITY (ordinals, u32 scores, f32 bits, hit counts, padding): the
C oracle, and the staged two-launch path reached by calls of fewer than kWalkMinQueries queries. The chunk totals the
cases are named after are asserted from the census of the index FILE.

CPU: the constants the chunk arithmetic restates are the ones in the source text."""
import os
import re

import numpy as np
import pytest

from tests import accum_ref as ar
from tests import helpers

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mllm_sparse_retrieval_amd", "csrc")
WALK_MAX_TILES, WALK_MAX_K, WALK_MIN_QUERIES = 8, 64, 1024
UL = 4                  # LightChunks::UL: chunk loads per wave held across the selection
NQ = 1100
KS = (1, 10, 64)
BIG = 2048              # postings of a `big` term in a tile: 512 vecs = 8 chunks; 2048 / 4096 < DENSITY
BIG_CHUNKS = 8
DENSITY = 0.55          # dense-head density passed to build(): only `dense` (60 % of every tile) reaches it
TIE_DOCS = 600          # equal-scored docs in one tile: more than theta_select's 512-key candidate buffer holds


@pytest.fixture(scope="module")
def m(built):
    import mllm_sparse_retrieval_amd as m

    return m


def chunk_sequences(nw):
    """name -> chunk totals of the query in tiles 0, 1, 2 (repeated over the tiles of longer corpora). NW waves take
    chunks round-robin; a wave's first UL chunks are prefetched, so UL * NW is the most a tile holds without the
    leftover loop."""
    full, many = UL * nw, 3 * UL * nw + 2
    return {
        "many, 0, many": [many, 0, many],
        "0, many, 1": [0, many, 1],
        "UL*NW, UL*NW+1, 1": [full, full + 1, 1],
        "every tile above UL*NW": [full + 1, many, full + 1],
        "NW, NW+1, 0": [nw, nw + 1, 0],
        "1, NW, NW+1": [1, nw, nw + 1],
    }


def corpus(tile_docs, n_docs, seed=0):
    """Terms by role (ids in `roles`):
        dense      60 % of every tile's docs: the only term of the dense head
        seq[name]  the terms of one chunk sequence: `big` terms of 8 chunks and `one` terms of 1 chunk, present in
                   exactly the tiles where the sequence needs them (tile t takes the totals of position t % 3)
        not0       40 docs in every tile but the first;  only_last  up to 30 docs of the last tile
        low        weight 1 on 100 docs of tile 0: fills the running top-k below every tied doc
        mass       weight 9 on TIE_DOCS docs of tile 1 and on 3 docs of tile 0
        mass_last  the same with the tied docs in the last tile
        fill       40 terms of 1-8 docs per tile"""
    rng = np.random.default_rng(777 + seed)
    sizes = [min(tile_docs, n_docs - t * tile_docs) for t in range(-(-n_docs // tile_docs))]
    T = len(sizes)
    nw = ar.INSTANCES[tile_docs][0] // 64
    roles, counts, explicit, at = {"seq": {}}, {}, {}, 0

    def new():
        nonlocal at
        at += 1
        return at - 1

    roles["dense"] = new()
    counts[roles["dense"]] = [max(1, int(0.6 * nd)) for nd in sizes]
    for name, tot in chunk_sequences(nw).items():
        per_tile = [tot[t % 3] for t in range(T)]
        n_big, n_one = max(x // BIG_CHUNKS for x in per_tile), max(x % BIG_CHUNKS for x in per_tile)
        terms = []
        for i in range(n_big):
            terms.append(new())
            counts[terms[-1]] = [min(BIG, nd) if i < x // BIG_CHUNKS else 0 for x, nd in zip(per_tile, sizes)]
        for j in range(n_one):
            terms.append(new())
            counts[terms[-1]] = [min(5 + j, nd) if j < x % BIG_CHUNKS else 0 for x, nd in zip(per_tile, sizes)]
        roles["seq"][name] = terms
    roles["not0"] = new()
    counts[roles["not0"]] = [0] + [min(40, nd) for nd in sizes[1:]]
    roles["only_last"] = new()
    counts[roles["only_last"]] = [0] * (T - 1) + [min(30, sizes[-1])]
    roles["low"] = new()
    explicit[roles["low"]] = (np.sort(rng.choice(np.arange(100, sizes[0]), size=100, replace=False)).tolist(), [1] * 100)
    for name, tile in (("mass", 1), ("mass_last", T - 1)):
        n_mass = min(TIE_DOCS, sizes[tile])
        rows = [20, 21, 22] + (tile * tile_docs + np.sort(rng.choice(sizes[tile], size=n_mass, replace=False))).tolist()
        roles[name] = new()
        explicit[roles[name]] = (rows, [9] * len(rows))
    roles["fill"] = []
    for _ in range(40):
        roles["fill"].append(new())
        counts[roles["fill"][-1]] = [min(int(c), nd) for c, nd in zip(rng.integers(1, 9, size=T), sizes)]
    p = ar.plant(tile_docs, n_docs, at, counts, explicit=explicit, seed=seed)
    p.update(roles=roles, sizes=sizes, nw=nw)
    return p


def queries(p, seed=0):
    """NQ queries: the named cases first, then seeded mixes of the corpus' terms -> (csr, {name: query index})."""
    r, rng = p["roles"], np.random.default_rng(31 + seed)
    named = {}
    for name, terms in r["seq"].items():
        ents = [(t, 1 + i % 5) for i, t in enumerate(terms)]
        named[name] = ents
        named[name + " + dense head"] = [(r["dense"], 2)] + ents
    named.update({
        "no hit in the first tile": [(r["not0"], 3)],
        "overflow in tile 1": [(r["low"], 1), (r["mass"], 2)],
        "overflow in the last tile": [(r["low"], 1), (r["mass_last"], 2)],
        "hits only in the last tile": [(r["only_last"], 4)],
        "dense head only": [(r["dense"], 3)],
        "no terms": [],
    })
    qs, where = list(named.values()), {n: i for i, n in enumerate(named)}
    pool = [r["dense"], r["not0"], r["only_last"], r["low"]] + r["fill"] + [t for ts in r["seq"].values() for t in ts]
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


def check_census(p, cen, where):
    """The chunk totals the sequence cases are named after (three full tiles), from the index file."""
    for name, tot in chunk_sequences(p["nw"]).items():
        for qname in (name, name + " + dense head"):
            got = [t["total_chunks"] for t in cen["queries"][where[qname]]["tiles"]]
            assert got == tot, (qname, got)
            assert cen["queries"][where[qname]]["pairs"] == int(qname.endswith("dense head"))
    full = UL * p["nw"]
    seen = {x for tot in chunk_sequences(p["nw"]).values() for x in tot}
    assert seen == {0, 1, p["nw"], p["nw"] + 1, full, full + 1, 3 * full + 2}


def self_check(p, where, want):
    """What the selection cases reach at k = 10, from the oracle's result."""
    w_ord, w_sc, w_n = want
    T, td = len(p["sizes"]), p["tile_docs"]
    assert w_n[where["no terms"]] == 0
    i = where["no hit in the first tile"]
    assert w_n[i] == min(10, sum(min(40, nd) for nd in p["sizes"][1:])) and (w_ord[i, :w_n[i]] >= td).all()
    i = where["hits only in the last tile"]
    assert w_n[i] == min(10, 30, p["sizes"][-1]) and (w_ord[i, :w_n[i]] >= (T - 1) * td).all()
    for name, tile in (("overflow in tile 1", 1), ("overflow in the last tile", T - 1)):
        if p["sizes"][tile] < TIE_DOCS:
            continue
        i = where[name]
        # tile 0 fills the top-10 (3 tied docs, then `low` docs); all TIE_DOCS tied docs of `tile` beat its 10th key
        assert w_n[i] == 10 and (w_ord[i, :3] < td).all() and len(np.unique(w_sc[i])) == 1
        assert (w_ord[i, 3:] >= tile * td).all() and (w_ord[i, 3:] < (tile + 1) * td).all()


# (name, tile_docs, docs, three full tiles: the chunk sequences are asserted)
SHAPES = [("3 tiles of 4096", 4096, 3 * 4096, True), ("3 tiles of 8192", 8192, 3 * 8192, True),
          ("2 tiles, one doc in the last", 8192, 8193, False), ("8 tiles of 4096", 4096, 7 * 4096 + 1, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,tile_docs,n_docs,sequences", SHAPES, ids=[s[0].replace(" ", "_").replace(",", "") for s in SHAPES])
def test_prefetching_walk_equals_oracle_and_staged_path(m, tmp_path, name, tile_docs, n_docs, sequences):
    p = corpus(tile_docs, n_docs)
    path = ar.build(m, tmp_path / "w.idx", p, 1, DENSITY)
    oix, _ = helpers.taat_oracle(p["docs"], p["n_terms"], p["ids"])
    q, where = queries(p)
    cen = ar.census(path, q, 10)
    assert cen["batch"]["light"] and cen["ix"]["n_dense"] == 2 and cen["batch"]["NW"] == p["nw"]
    assert int(cen["ix"]["dense_terms"][0]) == p["roles"]["dense"]
    assert cen["queries"][where["dense head only"]]["dense_only"]
    assert cen["queries"][where["no terms"]]["n_sparse"] == 0 and not cen["queries"][where["no terms"]]["pairs"]
    assert all(c["error"] is None for c in cen["queries"])
    if sequences:
        check_census(p, cen, where)
        assert [t["total_chunks"] for t in cen["queries"][where["no hit in the first tile"]]["tiles"]] == [0, 1, 1]
    with m.SparseIndex(path, device=0) as ix:
        assert ix.n_tiles == len(p["sizes"]) and 2 <= ix.n_tiles <= WALK_MAX_TILES
        b = ix.batch(*q, 65)
        try:
            for n_walked, k in enumerate(KS, start=1):
                want = oix.search(*q, k, threads=8)
                if k == 10:
                    self_check(p, where, want)
                b.search(k)
                got = b.fetch()
                assert int(b.debug_stamps()[7]) == n_walked, (name, k)      # the route
                helpers.assert_same_results(got, want, k)
                _equal(got, _staged(ix, q, k))
            b.search(WALK_MAX_K + 1)                                         # k = 65 stays on the staged path
            got = b.fetch()
            assert int(b.debug_stamps()[7]) == len(KS)
            helpers.assert_same_results(got, oix.search(*q, WALK_MAX_K + 1, threads=8), WALK_MAX_K + 1)
            assert b.debug_stamps()[:7].sum() == 0
        finally:
            b.close()


# ------------------------------------------------------------------------------------------------------ CPU
def test_pipeline_constants_are_the_source_text():
    def src(name):
        with open(os.path.join(CSRC, name), encoding="utf-8") as f:
            return f.read()

    internal, acc, walk = src("msr_device_internal.hpp"), src("msr_accumulate.hpp"), src("msr_walk.hpp")
    assert re.search(rf"constexpr uint32_t kWalkMaxTiles = {WALK_MAX_TILES};", internal)
    assert re.search(rf"constexpr uint32_t kWalkMaxK = {WALK_MAX_K};", internal)
    assert re.search(rf"constexpr uint32_t kWalkMinQueries = {WALK_MIN_QUERIES};", internal)
    assert f"static constexpr int UL = {UL};" in acc and UL == ar.UL
    assert "constexpr int CAND = 512;" in walk and TIE_DOCS > 512
    assert "LightChunks<NT / 64> ch;" in walk                               # NW waves share a tile's chunks
    assert [ar.INSTANCES[t][0] // 64 for t in ar.LIGHT_TILES] == [4, 8]
    assert ar.CHUNK_VECS * 4 * BIG_CHUNKS == BIG and BIG / min(ar.LIGHT_TILES) < DENSITY
