"""Planted corpora, a boundary census and a numpy reference for the sparse accumulation (csrc/msr_accumulate.hpp:
accumulate_tile, accumulate_tile_light) and the selection behind it (csrc/msr_select.hpp: tile_select).

plant()   a doc-major CSR whose (tile, term) posting counts, weights and dense-head membership are chosen, not drawn.
census()  from the index FILE (helpers.read_index_file) and the query CSR alone: the host normalisation of
          batch_create_impl restated, and per query and tile the quantities the kernels branch on. A GPU case asserts
          the census facts it is named after before it searches, so a case that stops reaching its edge fails on any
          machine (tests/test_accum_ref.py lists every edge by name).
numpy_scores() + rank()  int64 D @ q ranked with np.lexsort((ordinal, -score)): the second reference beside the C
          oracle.

Nothing here calls the search path of libmsr; only build() calls the index builder. When an accumulation constant
changes (kQtBlock, kChunkVecs, UL, the tile shapes of with_tile_shape), this is the file to restate it in:
tests/test_accum_ref.py compares INSTANCES with the source text of the table's TileShape rows."""
from __future__ import annotations

import numpy as np

from tests import helpers

KQT_BLOCK = 256      # kQtBlock: sparse query entries staged per round
CHUNK_VECS = 64      # kChunkVecs: one chunk = 64 vecs = 256 postings = 1 KiB
UL = 4               # accumulate_tile_light: chunk loads per wave and batch
LIGHT_MAX = 64       # batch_search_local: the light path takes batches whose queries hold at most 64 sparse entries
LIGHT_TILES = (4096, 8192)
# with_tile_shape's table (msr_device_internal.hpp): tile_docs -> (threads NT, chunk loads per register bank U)
INSTANCES = {32768: (1024, 8), 16384: (512, 8), 12288: (512, 4), 8192: (512, 4), 4096: (256, 4)}
TILE_SIZES = sorted(INSTANCES)
NO_TERM = 0xFFFFFFFF


def instance(tile_docs, k, light_batch):
    """The score_tiles instance launch_score picks for (tile size, k) and a batch that is light or not."""
    nt, u = INSTANCES[tile_docs]
    return dict(NT=nt, NW=nt // 64, U=u, CAND=512 if k <= 512 else 1024,
                light=bool(light_batch and k <= 512 and tile_docs in LIGHT_TILES), R=tile_docs // (4 * nt))


# ------------------------------------------------------------------------------------------------------ planting
def plant(tile_docs, n_docs, n_terms, counts, weights=None, explicit=None, seed=0):
    """counts: {term: [postings in tile 0, tile 1, ...]} placed on a seeded random subset of each tile's docs (all of
    them when the count is the tile's size), weights drawn from weights[term] = (lo, hi), default (1, 255).
    explicit: {term: (global doc rows, weights)} for terms placed by hand.
    -> dict(docs=(dp, dt, dw), ids, n_terms, n_docs, tile_docs, per=int [n_tiles, n_terms] planted counts).
    Doc ids are zero-padded decimals, so ordinal == row and "tile" means rows [tile * tile_docs, ...)."""
    rng = np.random.default_rng(seed)
    n_tiles = (n_docs + tile_docs - 1) // tile_docs
    per = np.zeros((n_tiles, n_terms), dtype=np.int64)
    d_all, t_all, w_all = [], [], []
    for t in sorted(counts):
        lo, hi = (weights or {}).get(t, (1, 255))
        for tile, c in enumerate(counts[t]):
            nd = min(tile_docs, n_docs - tile * tile_docs)
            assert 0 <= c <= nd, (t, tile, c, nd)
            if c == 0:
                continue
            loc = np.arange(nd) if c == nd else rng.choice(nd, size=c, replace=False)
            d_all.append(tile * tile_docs + loc.astype(np.int64))
            t_all.append(np.full(c, t, dtype=np.int64))
            w_all.append(rng.integers(lo, hi + 1, size=c))
            per[tile, t] = c
    for t, (rows, w) in sorted((explicit or {}).items()):
        rows = np.asarray(rows, dtype=np.int64)
        assert t not in counts and len(np.unique(rows)) == len(rows) == len(w) and (np.asarray(w) > 0).all()
        d_all.append(rows)
        t_all.append(np.full(len(rows), t, dtype=np.int64))
        w_all.append(np.asarray(w, dtype=np.int64))
        per[:, t] = np.bincount(rows // tile_docs, minlength=n_tiles)
    d, t, w = np.concatenate(d_all), np.concatenate(t_all), np.concatenate(w_all)
    order = np.lexsort((t, d))
    dp = np.concatenate([[0], np.cumsum(np.bincount(d, minlength=n_docs))]).astype(np.uint64)
    return dict(docs=(dp, t[order].astype(np.uint32), w[order].astype(np.uint32)), n_terms=n_terms, n_docs=n_docs,
                tile_docs=tile_docs, ids=[f"{i:07d}" for i in range(n_docs)], per=per)


def build(m, path, planted, dense_max_terms=0, dense_min_density=0.4):
    """Index file of a planted corpus with the dense head steered by the build options (restored afterwards)."""
    m.set_build_option("dense_max_terms", dense_max_terms)
    m.set_build_option("dense_min_density", dense_min_density)
    try:
        return m.build_index_from_csr(str(path), *planted["docs"], planted["n_terms"], doc_ids=planted["ids"],
                                      tile_docs=planted["tile_docs"])
    finally:
        m.set_build_option("dense_max_terms", 16)
        m.set_build_option("dense_min_density", 0.4)


def segment_postings(ix):
    """Real (weight != 0) postings per (tile, term) of a decoded index file -> int [n_tiles, n_terms]."""
    cs = np.concatenate([[0], np.cumsum((ix["postings"] >> 16) != 0)])
    sp = ix["seg_ptr"].astype(np.int64) * 4
    return cs[sp[:, 1:]] - cs[sp[:, :-1]]


def csr(queries):
    """[[(term, weight), ...], ...] -> (q_ptr int64, q_term int32, q_w int32)."""
    qp = np.concatenate([[0], np.cumsum([len(q) for q in queries])]).astype(np.int64)
    qt = np.array([t for q in queries for t, _ in q], dtype=np.int32)
    qw = np.array([w for q in queries for _, w in q], dtype=np.int32)
    return qp, qt, qw


# -------------------------------------------------------------------------------------------------------- census
def normalise(ix, entries, drop_df_eq_n=True):
    """batch_create_impl's walk over one query's (term, weight) entries, in its order of checks.
    -> dict(error None | 'RANGE' | 'OVERFLOW', sparse [(term, w)], dsum per dense slot, bound)."""
    dense_slot = {int(t): s for s, t in enumerate(ix["dense_terms"]) if t != NO_TERM}
    sparse, dsum, bound = [], [0] * int(ix["n_dense"]), 0
    for t, w in entries:
        t, w = int(t), int(w)
        if t < 0 or w <= 0:
            continue
        if t >= ix["n_terms"] or w > 0xFFFFFF:
            return dict(error="RANGE", sparse=sparse, dsum=dsum, bound=bound)
        df = int(ix["df"][t])
        if (drop_df_eq_n and df == ix["n_docs"]) or df == 0:
            continue
        bound += w * int(ix["maxw"][t])
        if t in dense_slot:
            if dsum[dense_slot[t]] + w > 0xFFFF:
                return dict(error="RANGE", sparse=sparse, dsum=dsum, bound=bound)
            dsum[dense_slot[t]] += w
        else:
            sparse.append((t, w))  # repeated sparse terms stay separate entries
    return dict(error="OVERFLOW" if bound > 0xFFFFFFFF else None, sparse=sparse, dsum=dsum, bound=bound)


def census(index_file, queries, k, drop_df_eq_n=True):
    """queries: (q_ptr, q_term, q_w). -> dict(batch=..., queries=[...]); see the module docstring.
    Per query: error, n_sparse, entries_per_round, pairs, halves {pair: 'lo' | 'hi' | 'both'}, dense_only, bound,
    tiles = [dict(ndocs, rounds, postings, vecs, chunks, tails, zero_at, total_chunks, chunks_per_round,
    chunks_per_wave [round][wave], last_segment)] with one list entry per sparse entry of the query.
    Per batch: max_sparse, light_batch, and the instance() of (tile size, k)."""
    ix = index_file if isinstance(index_file, dict) else helpers.read_index_file(index_file)
    qp, qt, qw = queries
    segp = segment_postings(ix)
    vecs_all = np.diff(ix["seg_ptr"].astype(np.int64), axis=1)
    norm = [normalise(ix, zip(qt[qp[i]:qp[i + 1]], qw[qp[i]:qp[i + 1]]), drop_df_eq_n) for i in range(len(qp) - 1)]
    max_sparse = max([len(n["sparse"]) for n in norm if n["error"] is None], default=0)
    inst = instance(ix["tile_docs"], k, max_sparse <= LIGHT_MAX)
    nw, nt = inst["NW"], inst["NT"]
    out = []
    for n in norm:
        terms = np.array([t for t, _ in n["sparse"]], dtype=np.int64)
        ns = len(terms)
        halves = {}
        for s, w in enumerate(n["dsum"]):
            if w:
                halves[s // 2] = "both" if s // 2 in halves else ("hi" if s & 1 else "lo")
        tiles = []
        for tile in range(ix["n_tiles"]):
            ndocs = min(ix["tile_docs"], ix["n_docs"] - tile * ix["tile_docs"])
            vecs = vecs_all[tile, terms] if ns else np.zeros(0, np.int64)
            chunks = (vecs + CHUNK_VECS - 1) // CHUNK_VECS
            per_round = [int(chunks[b:b + KQT_BLOCK].sum()) for b in range(0, ns, KQT_BLOCK)]
            tiles.append(dict(
                ndocs=int(ndocs), rounds=int((ndocs + 4 * nt - 1) // (4 * nt)),
                postings=[int(x) for x in (segp[tile, terms] if ns else [])], vecs=[int(x) for x in vecs],
                chunks=[int(x) for x in chunks],
                tails=[int(v - (c - 1) * CHUNK_VECS) if c else 0 for v, c in zip(vecs, chunks)],  # vecs of the last chunk
                zero_at=[i for i, c in enumerate(chunks) if c == 0], total_chunks=int(chunks.sum()),
                chunks_per_round=per_round,
                chunks_per_wave=[[(tot - w + nw - 1) // nw if tot > w else 0 for w in range(nw)] for tot in per_round],
                last_segment=bool(ns and vecs[-1] > 0 and tile == ix["n_tiles"] - 1
                                  and int(ix["seg_ptr"][tile, terms[-1] + 1]) == ix["n_vecs"])))
        out.append(dict(error=n["error"], n_sparse=ns, bound=n["bound"], dsum=n["dsum"],
                        entries_per_round=[min(KQT_BLOCK, ns - b) for b in range(0, ns, KQT_BLOCK)],
                        pairs=len(halves), halves=halves, dense_only=bool(ns == 0 and halves), tiles=tiles))
    return dict(batch=dict(max_sparse=max_sparse, light_batch=max_sparse <= LIGHT_MAX, **inst), queries=out, ix=ix)


def check_fact(cen, qi, fact):
    """One census fact of query qi, as a case states it: (kind, args...). Raises AssertionError with the census value."""
    q, b = cen["queries"][qi], cen["batch"]
    kind, a = fact[0], fact[1:]
    if kind == "postings":       # (tile, [counts]): the real postings of the query's first len(counts) segments
        got = q["tiles"][a[0]]["postings"][:len(a[1])]
        want = list(a[1])
        assert [-(-x // 4) for x in want] == q["tiles"][a[0]]["vecs"][:len(want)], (fact, q["tiles"][a[0]]["vecs"][:len(want)])
    elif kind == "n_sparse":
        got, want = q["n_sparse"], a[0]
    elif kind == "entries_per_round":
        got, want = q["entries_per_round"], list(a[0])
    elif kind == "zero_at":      # (tile, [positions of the query's entries whose segment is empty in the tile])
        got, want = q["tiles"][a[0]]["zero_at"], list(a[1])
    elif kind == "total_chunks":  # (tile, chunks of the whole workgroup)
        got, want = q["tiles"][a[0]]["total_chunks"], a[1]
    elif kind == "wave_chunks":  # (tile, round, chunks of wave 0 in that round): the general path's c_end
        got, want = q["tiles"][a[0]]["chunks_per_wave"][a[1]][0], a[2]
        assert not b["light"], fact
    elif kind == "last_segment":
        got, want = q["tiles"][-1]["last_segment"], True
    elif kind == "pairs":
        got, want = q["pairs"], a[0]
    elif kind == "halves":
        got, want = q["halves"], dict(a[0])
    elif kind == "dense_only":
        got, want = q["dense_only"], True
    elif kind == "dsum":         # (slot, summed 16-bit query weight)
        got, want = q["dsum"][a[0]], a[1]
    elif kind == "last_tile":    # (docs, rounds) of the corpus' last tile
        got, want = (q["tiles"][-1]["ndocs"], q["tiles"][-1]["rounds"]), tuple(a)
    elif kind == "dense_in_last_tile":  # dense slot 0 (which the query holds) has a posting in the last tile
        got, want = (bool((cen["ix"]["dense"][-1, 0, :] & 0xFFFF).any()), q["dsum"][0] > 0), (True, True)
    elif kind == "padded_slot":  # odd dense_max_terms: the last slot is padding and the query holds its pair
        got, want = (int(cen["ix"]["dense_terms"][-1]), len(cen["ix"]["dense_terms"]) // 2 - 1 in q["halves"]), (NO_TERM, True)
    else:
        raise KeyError(kind)
    assert got == want, (fact, got)


# ---------------------------------------------------------------------------------------------- numpy reference
def numpy_scores(ix, D, queries, drop_df_eq_n=True):
    """int64 D @ q over the dense matrix of the index file -> scores [nq, n_docs]."""
    qp, qt, qw = queries
    DT = np.ascontiguousarray(D.T)
    S = np.zeros((len(qp) - 1, D.shape[0]), dtype=np.int64)
    for i in range(len(qp) - 1):
        for t, w in zip(qt[qp[i]:qp[i + 1]], qw[qp[i]:qp[i + 1]]):
            if t < 0 or w <= 0 or (drop_df_eq_n and ix["df"][t] == ix["n_docs"]):
                continue
            S[i] += DT[t] * int(w)
    assert S.max(initial=0) <= 0xFFFFFFFF
    return S


def rank(S, k):
    """Scores [nq, n_docs] ranked by (score descending, ordinal ascending), hits are the docs with a positive score
    -> (ords int64 [nq, k] padded -1, scores int64 padded 0, n int32): the oracle's shape."""
    nq = S.shape[0]
    ords = np.full((nq, k), -1, dtype=np.int64)
    sc = np.zeros((nq, k), dtype=np.int64)
    n = np.zeros(nq, dtype=np.int32)
    for i, s in enumerate(S):
        order = np.lexsort((np.arange(len(s)), -s))[:k]
        order = order[s[order] > 0]
        ords[i, :len(order)], sc[i, :len(order)], n[i] = order, s[order], len(order)
    return ords, sc, n


def select_path(scores, tile_docs, k):
    """Which selection tile_select runs on one tile's accumulators `scores` (int64), where that follows from the
    scores alone: 'empty' (no positive score), 'direct' (the candidates fit the CAND-key buffer whatever tau0 is),
    'hist' / 'radix' (more than CAND accumulators reach the k-th largest score — every lower bound tau0 keeps them
    all — or k > NT, where tau0 = 1 keeps every positive one: hist_threshold for tiles <= 8192 docs with the
    1024-key buffer, else the byte-wise radix passes), 'open' (depends on the 8-bit rounding of tau0)."""
    nt = INSTANCES[tile_docs][0]
    cand = 512 if k <= 512 else 1024
    pos = np.sort(scores[scores > 0])[::-1]
    if len(pos) == 0:
        return "empty"
    if len(pos) <= cand:
        return "direct"
    kth = int(pos[k - 1]) if len(pos) >= k else 1
    if k > nt or int((pos >= kth).sum()) > cand:
        return "hist" if tile_docs <= 8192 and cand == 1024 else "radix"
    return "open"


def switch_of(tile_docs, k):
    """tile_select's tau0 branch for k."""
    return "k<=64" if k <= 64 else ("k<=NT" if k <= INSTANCES[tile_docs][0] else "k>NT")


# ------------------------------------------------------------------------------------------- geometry case lists
M_COUNTS = [1, 3, 4, 5, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025]  # + tile_docs - 1, tile_docs without a dense head
N_FILL = 300
ENTRY_COUNTS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513]
WAVE_CHUNKS = ["1", "U", "U+1", "2U", "2U+1", "64", "65"]
LIGHT_CHUNKS = ["NW-1", "NW", "NW+1", "UL*NW", "UL*NW+1", ">2*UL*NW"]
LAST_TILES = ["1", "4NT-1", "4NT", "4NT+1", "R-1 rounds"]
DENSE_DENSITY = 0.55  # only the planted dense terms reach it (see geometry_corpus)


def last_tile_docs(tile_docs, label):
    nt = INSTANCES[tile_docs][0]
    return {"1": 1, "4NT-1": 4 * nt - 1, "4NT": 4 * nt, "4NT+1": 4 * nt + 1,
            "R-1 rounds": (tile_docs // (4 * nt) - 1) * 4 * nt}[label]


def geometry_corpus(tile_docs, last_label="R-1 rounds", n_dense=0, n_full=1, seed=0):
    """`n_full` full tiles and a last tile of last_tile_docs(last_label) docs. Terms, in id order:
        m-terms     one per planted segment length; term i holds m[(i + 5 * tile) % len(m)] postings in `tile`
        a0, a1      absent from tile 0 (40 postings elsewhere);  b  absent from the last tile (40 in the others)
        dense       `n_dense` terms held by 62-100 % of every tile's docs, distinct df descending with the id: the only
                    terms at or above DENSE_DENSITY, so slot s of the dense head is dense[s] (with a dense head the
                    m-terms stop at 1025 postings: a full-tile segment would outrank them)
        fillers     N_FILL terms of 1-8 postings per tile (one chunk each)
        last        5 postings per tile: its segment ends the last tile and the postings array
    -> planted dict + roles (term ids by name)."""
    last = last_tile_docs(tile_docs, last_label)
    sizes = [tile_docs] * n_full + [last]
    n_docs = sum(sizes)
    m = M_COUNTS + ([] if n_dense else [tile_docs - 1, tile_docs])
    rng = np.random.default_rng(1000 + seed)
    counts, at = {}, 0
    roles = dict(m={}, m_list=m)
    for i, mv in enumerate(m):
        counts[at] = [min(m[(i + 5 * t) % len(m)], nd) for t, nd in enumerate(sizes)]
        if sum(counts[at]) == n_docs:   # (a one-doc last tile: df == N would drop the full-tile term from every query)
            counts[at][-1] = 0
        roles["m"][mv] = at
        at += 1
    for name in ("a0", "a1"):
        counts[at] = [0] + [min(40, nd) for nd in sizes[1:]]
        roles[name] = at
        at += 1
    counts[at] = [40] * n_full + [0]
    roles["b"] = at
    at += 1
    roles["dense"] = list(range(at, at + n_dense))
    for i in range(n_dense):
        counts[at] = [max(nd - 1 - i * (nd // 80), 0) for nd in sizes]
        if i == 0 and sizes[-1] == 1:   # a one-doc last tile: its doc holds the first dense term, so the row there counts
            counts[at][-1] = 1
        at += 1
    roles["fill"] = list(range(at, at + N_FILL))
    for i in range(N_FILL):
        counts[at] = [min(int(c), nd) for c, nd in zip(rng.integers(1, 9, size=len(sizes)), sizes)]
        at += 1
    counts[at] = [min(5, nd) for nd in sizes]
    roles["last"] = at
    at += 1
    p = plant(tile_docs, n_docs, at, counts, seed=seed)
    p.update(roles=roles, sizes=sizes, n_dense_planted=n_dense, last_label=last_label)
    return p


def _compose(pool, target, max_entries):
    """Entries (term ids, repeats allowed, distinct terms first) whose chunk counts in `pool` {term: chunks} add up
    to `target`: every multi-chunk term once while it fits, then always the longest segment that still fits, taking
    turns among the terms of that length."""
    by = sorted(pool.items(), key=lambda kv: (-kv[1], kv[0]))
    out, left = [], target
    for t, c in by:
        if 1 < c <= left:
            out.append(t)
            left -= c
    turn = {}
    while left > 0:
        c = max(c for _, c in by if c <= left)
        same = [t for t, c2 in by if c2 == c]
        out.append(same[turn.get(c, 0) % len(same)])
        turn[c] = turn.get(c, 0) + 1
        left -= c
    assert len(out) <= max_entries, (target, len(out))
    return out


class Case:
    """One query of a case list: the edges it is named after, its (term, weight) entries, and the census facts that
    prove it reaches them."""

    def __init__(self, edges, entries, *facts):
        self.edges = [edges] if isinstance(edges, str) else list(edges)
        self.entries = list(entries)
        self.facts = list(facts)


def geometry_cases(p):
    """-> (light cases, general-only cases). The light list holds at most 64 sparse entries per query, so a batch of
    it alone takes accumulate_tile_light where the instance has one; the general batch is the light list PLUS the
    general-only cases (one query above 64 entries moves the whole batch to accumulate_tile)."""
    r, T = p["roles"], p["tile_docs"]
    nt, u = INSTANCES[T]
    nw = nt // 64
    fill, m_ids = r["fill"], r["m"]
    per0 = p["per"][0]
    chunks0 = {t: int(-(-int(per0[t]) // 256)) for t in list(m_ids.values()) + fill}
    w = lambda i: 1 + i % 5
    light, general = [], []
    # segment lengths, alone and together
    for mv, t in m_ids.items():
        light.append(Case(f"m={_mname(mv, T)} alone", [(t, 2)], ("postings", 0, [mv]), ("n_sparse", 1)))
    light.append(Case([f"m={_mname(mv, T)} multi" for mv in m_ids], [(t, w(i)) for i, t in enumerate(m_ids.values())]
                      + [(fill[0], 2), (fill[1], 1)], ("postings", 0, list(m_ids)), ("n_sparse", len(m_ids) + 2)))
    light.append(Case("last segment of the postings array", [(fill[2], 1), (r["last"], 3)], ("last_segment",)))
    # absent terms (tile 0)
    x, y = fill[3], fill[4]
    light.append(Case("absent first", [(r["a0"], 2), (x, 1), (y, 3)], ("zero_at", 0, [0])))
    light.append(Case("absent middle", [(x, 1), (r["a0"], 2), (y, 3)], ("zero_at", 0, [1])))
    light.append(Case("absent last", [(x, 1), (y, 3), (r["a0"], 2)], ("zero_at", 0, [2])))
    light.append(Case("absent everywhere", [(r["a0"], 2), (r["a1"], 1)], ("zero_at", 0, [0, 1]), ("total_chunks", 0, 0)))
    light.append(Case("absent from the last tile", [(x, 2), (r["b"], 1)], ("zero_at", len(p["sizes"]) - 1, [1])))
    # entries per query
    for n in ENTRY_COUNTS:
        ents = [(fill[(7 * i) % N_FILL], w(i)) for i in range(n)]
        rounds = [min(256, n - b) for b in range(0, n, 256)]
        (light if n <= LIGHT_MAX else general).append(
            Case(f"entries={n}", ents, ("n_sparse", n), ("entries_per_round", rounds)))
    light.append(Case("repeated term", [(fill[5], 3), (fill[5], 4), (m_ids[257], 1), (fill[5], 5), (m_ids[257], 2)],
                      ("n_sparse", 5), ("postings", 0, [int(per0[fill[5]])] * 2 + [257, int(per0[fill[5]]), 257])))
    # light path: chunks per workgroup
    if T in LIGHT_TILES:
        for label, tot in zip(LIGHT_CHUNKS, [nw - 1, nw, nw + 1, UL * nw, UL * nw + 1, 2 * UL * nw + 5]):
            ents = [(t, w(i)) for i, t in enumerate(_compose(chunks0, tot, LIGHT_MAX) if tot > LIGHT_MAX
                                                    else fill[10:10 + tot])]
            light.append(Case(f"light chunks={label}", ents, ("total_chunks", 0, tot)))
    # general path: chunks per wave in one round
    for label, c in zip(WAVE_CHUNKS, [1, u, u + 1, 2 * u, 2 * u + 1, 64, 65]):
        tot = c * nw
        ents = [(t, w(i)) for i, t in enumerate(_compose(chunks0, tot, KQT_BLOCK) if tot > 200 else fill[20:20 + tot])]
        general.append(Case(f"wave chunks={label}", ents, ("wave_chunks", 0, 0, c), ("entries_per_round", [len(ents)])))
    # dense head
    d = r["dense"]
    if d:
        n_pairs = (len(d) + 1) // 2
        sparse3 = [(fill[6], 2), (m_ids[257], 1), (fill[7], 3)]
        light.append(Case("half=lo", [(d[0], 3)] + sparse3, ("halves", {0: "lo"}), ("pairs", 1)))
        light.append(Case("half=hi", [(d[1], 3)] + sparse3, ("halves", {0: "hi"})))
        light.append(Case(["half=both", "dense only"], [(d[0], 2), (d[1], 5)], ("halves", {0: "both"}), ("dense_only",)))
        for n in (1, 2, 3, 4, 5, 16):
            if n > n_pairs:
                continue
            ents = [(d[min(2 * q + q % 2, len(d) - 1)], 1 + q % 7) for q in range(n)]
            light.append(Case(f"pairs={n}", ents + sparse3, ("pairs", n), ("n_sparse", 3)))
            general.append(Case(f"pairs={n} general", ents + [(fill[(11 * i) % N_FILL], w(i)) for i in range(70)],
                                ("pairs", n), ("n_sparse", 70)))
        light.append(Case("dense only, every slot", [(t, 1 + i % 9) for i, t in enumerate(d)], ("dense_only",),
                          ("pairs", n_pairs)))
        light.append(Case("dense weight sums to 65535", [(d[0], 30000), (x, 1), (d[0], 30000), (d[0], 5535)],
                          ("dsum", 0, 65535), ("n_sparse", 1)))
        if len(d) % 2:
            light.append(Case("padded slot", [(d[-1], 4), (x, 1)], ("padded_slot",), ("halves", {n_pairs - 1: "lo"})))
    nt_last = (p["sizes"][-1], -(-p["sizes"][-1] // (4 * nt)))
    tag = f"last tile={p['last_label']} " + ("with dense head" if d else "without dense head")
    light.append(Case(tag, ([(d[0], 2), (d[-1], 1)] if d else []) + [(r["last"], 2), (x, 1)], ("last_tile",) + nt_last,
                      *([("dense_in_last_tile",)] if d else [])))
    return light, general


def _mname(mv, tile_docs):
    return {tile_docs - 1: "T-1", tile_docs: "T"}.get(mv, str(mv))


def geometry_required(tile_docs, n_dense, last_label):
    """The edge names a geometry corpus' case lists must cover."""
    ms = [str(x) for x in M_COUNTS] + ([] if n_dense else ["T-1", "T"])
    req = [f"m={x} alone" for x in ms] + [f"m={x} multi" for x in ms]
    req += ["last segment of the postings array", "absent first", "absent middle", "absent last", "absent everywhere",
            "absent from the last tile", "repeated term"]
    req += [f"entries={n}" for n in ENTRY_COUNTS] + [f"wave chunks={c}" for c in WAVE_CHUNKS]
    if tile_docs in LIGHT_TILES:
        req += [f"light chunks={c}" for c in LIGHT_CHUNKS]
    if n_dense:
        n_pairs = (n_dense + 1) // 2
        req += ["half=lo", "half=hi", "half=both", "dense only", "dense only, every slot", "dense weight sums to 65535"]
        req += [f"pairs={n}" for n in (1, 2, 3, 4, 5, 16) if n <= n_pairs]
        req += [f"pairs={n} general" for n in (1, 2, 3, 4, 5, 16) if n <= n_pairs]
        if n_dense % 2:
            req.append("padded slot")
    req.append(f"last tile={last_label} " + ("with dense head" if n_dense else "without dense head"))
    return req


# (n_dense planted = dense_max_terms, last tile) of the geometry corpora every tile size goes through: the main shape
# without a dense head, with all 16 pairs and with an odd head; the other last-tile shapes with and without a head
GEOMETRY_VARIANTS = [(0, "R-1 rounds"), (32, "R-1 rounds"), (5, "R-1 rounds")] + \
                    [(nd, lab) for lab in LAST_TILES[:-1] for nd in (0, 32)]


# ----------------------------------------------------------------------------------- top of the score range
TOP_KS = [1, 64, 65, 256, 257, 512, 513, 1000, 1024]
W_CARRIER = 40000           # 65535 * 40000 = 2 621 400 000 >= 2^31
PLATEAU = 1500


def top_corpus(tile_docs, seed=0):
    """One full tile and 2000 more docs; scores in [2^31, 2^32). Terms:
        0 carrier   weight 65535 in every doc but the last (df = N - 1: kept under MSR_F_DROP_DF_EQ_N)
        1 distinct  (7919 * doc) % 60000 + 1 in every doc but the last: all different (n_docs < 60000, gcd = 1)
        2 plateau   weight 1 on PLATEAU seeded docs of tile 0
        3 rest      term 1's weights on the docs outside the plateau
        4 peak      65535 on doc 7, 65534 on doc tile_docs + 3
        5 bytes     weights 1-255 on a seeded half of the docs
        6 ones      weight 1 on three docs
        7 boost     weight 1 on 100 docs of tile 0 outside the plateau"""
    n = tile_docs + 2000
    rng = np.random.default_rng(77 + seed)
    body = np.arange(n - 1)
    distinct = (7919 * body) % 60000 + 1
    plateau = np.sort(rng.choice(tile_docs, size=PLATEAU, replace=False))
    outside = np.setdiff1d(body, plateau)
    half = np.sort(rng.choice(n, size=n // 2, replace=False))
    boost = np.sort(rng.choice(np.setdiff1d(np.arange(tile_docs), plateau), size=100, replace=False))
    explicit = {0: (body, np.full(n - 1, 65535)), 1: (body, distinct), 2: (plateau, np.ones(PLATEAU, np.int64)),
                3: (outside, distinct[outside]), 4: ([7, tile_docs + 3], [65535, 65534]),
                5: (half, rng.integers(1, 256, size=len(half))), 6: ([1, 2, tile_docs + 1], [1, 1, 1]),
                7: (boost, np.ones(100, np.int64))}
    p = plant(tile_docs, n, 8, {}, explicit=explicit, seed=seed)
    p.update(plateau=plateau, boost=boost)
    return p


# name -> entries; every bound sum w * maxw is at most 2^32 - 1
TOP_QUERIES = {
    "distinct": [(0, W_CARRIER), (1, 1)],
    "plateau top": [(0, W_CARRIER), (3, 1), (2, 60001)],
    "plateau mid": [(0, W_CARRIER), (3, 1), (2, 60001), (7, 61000)],
    "two scores": [(0, W_CARRIER), (2, 7)],
    "peak 0xFFFFFFFF": [(4, 65537)],
    "u24 weight 0xFFFFFF": [(5, 0xFFFFFF)],
    "65535 x 65535": [(0, 65535), (1, 1)],
    "65535 x 65535 tied": [(0, 32768), (0, 32767)],
}
TOP_GENERAL_EXTRA = [(6, 1)] * 65   # appended as one more query, it moves the batch to accumulate_tile
# (refused entries, error, accepted neighbour); the dense-head pair holds only where term 0 is in the dense head
TOP_REFUSALS = [
    ("sparse weight 0x1000000", [(5, 0x1000000)], "RANGE", [(5, 0xFFFFFF)]),
    ("bound 2^32", [(4, 65537), (6, 1)], "OVERFLOW", [(4, 65537)]),
]
TOP_REFUSAL_DENSE = ("dense-head weight 65536", [(0, 32768), (0, 32768)], "RANGE", [(0, 32768), (0, 32767)])


def hybrid_corpus(tile_docs, n_docs, seed=0):
    """Top-of-range corpus for the fused hybrid kernels: 0 carrier and 1 distinct as in top_corpus, 2 bytes = weights
    1-255 on a seeded half of the docs. Queries: three with distinct sparse scores, three whose sparse scores all lie
    within 255 of each other above 2^31 (the tight cluster: one or two f32 values for more than 512 docs)."""
    rng = np.random.default_rng(500 + seed)
    body = np.arange(n_docs - 1)
    half = np.sort(rng.choice(n_docs, size=n_docs // 2, replace=False))
    p = plant(tile_docs, n_docs, 3, {}, seed=seed, explicit={
        0: (body, np.full(n_docs - 1, 65535)), 1: (body, (7919 * body) % 60000 + 1),
        2: (half, rng.integers(1, 256, size=len(half)))})
    # (65535 * w = -w mod 256: with w = 40048 the f32 rounding midpoint falls at byte weight 240, inside the top of the
    # cluster, so its depth list holds two f32 values; with 40000 it holds one)
    p["queries"] = [[(0, W_CARRIER), (1, 1 + i)] for i in range(3)] + [[(0, w), (2, 1)] for w in (W_CARRIER, 40048, 40048)]
    p["tight"] = [3, 4, 5]
    return p


# what test_other_users_of_the_accumulation sends the three-tile corpora through, and the hybrid shapes
OTHER_USERS = dict(tile_docs=4096, n_full=2, n_dense=(0, 32), doc_shards=3, term_shards=(2, 3), ks=(10, 100))
HYBRID_SHAPES = [("single tile", 8192, 5000, 1), ("multi-tile", 4096, 10000, 0)]   # (name, tile, docs, dense_max_terms)
HYBRID_DEPTH = 300


def mixed_batch(light, general):
    """The light list plus ONE query above 64 entries (the entries=65 case): light except for that query."""
    extra = [c for c in general if c.edges == ["entries=65"]]
    assert len(extra) == 1
    return light + extra


def assert_hybrid_corpus(p, D, depth=HYBRID_DEPTH):
    """The facts the hybrid cases are named after, from the dense matrix of the built file: every depth list lies in
    [2^31, 2^32); the tight queries hold more than 512 docs within 255 of each other, their depth list more than two
    exact scores but at most two f32 values (both counts occur)."""
    f32_values = set()
    for i, ents in enumerate(p["queries"]):
        s = sum(D[:, t] * w for t, w in ents)
        top = np.sort(s)[::-1][:depth]
        assert 2**31 <= top.min() and top.max() < 2**32
        if i in p["tight"]:
            assert ((s > 0) & (s.max() - s <= 255)).sum() > 512
            assert len(np.unique(top)) > 2
            f32_values.add(len(np.unique(top.astype(np.float32))))
        else:
            assert len(np.unique(top.astype(np.float32))) > 2   # spread over several f32 values: no cluster
    assert f32_values == {1, 2}, f32_values


def top_variants():
    """(name, dense_max_terms, dense_min_density): the carrier in the dense head (v_dot2_u32_u16; one term, so its
    pair holds the padded slot) or in the inverted lists (__umul24 and the LDS atomics)."""
    return [("dense", 1, 0.9), ("sparse", 0, 0.4)]
