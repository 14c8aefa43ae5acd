"""msr_rank_docs on the GPU against the numpy reference of tests/rank_ref.py (S = Q @ D.T, ranks by the definition with
np.count_nonzero): exact equality of every rank and every u32 score, on the smallest shapes that reach each way the
rank kernels (csrc/msr_rank.hpp) can go wrong — several tiles with a ragged last one, every tile size with and without
a dense head, both accumulation paths, planted positions, mass ties across a tile boundary, scores with bit 31 set,
self_ord, the query split of the count phase — and against the search path and the CLI's own recall line."""
import os
import re

import numpy as np
import pytest

from tests import accum_ref as ar
from tests import helpers
from tests import rank_ref as rr

pytestmark = pytest.mark.gpu

E_INVAL, E_OVERFLOW = -1, -7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def m(built):
    import mllm_sparse_retrieval_amd as m

    return m


def sparse_entries(path, rows):
    """Kept entries outside the dense head per query: what picks the light (all <= 64) or the general accumulation."""
    f = helpers.read_index_file(str(path))
    dense = {int(t) for t in f["dense_terms"] if t != ar.NO_TERM}
    df, n = f["df"], f["n_docs"]
    return [sum(1 for t, w in r if t >= 0 and w > 0 and t not in dense and 0 < df[t] < n) for r in rows], dense


def check(ix, D, rows, targets, drop=True, self_ord=None):
    q, t = rr.csr(rows), rr.targets_csr(targets)
    want_r, want_s = rr.ranks(rr.scores(*q, D, drop), *t, self_ord)
    got_r, got_s = ix.rank_docs(*q, *t, drop_df_eq_n=drop, self_ord=self_ord)
    assert got_r.dtype == np.uint32 and got_s.dtype == np.uint32
    assert (got_s.astype(np.int64) == want_s).all(), np.flatnonzero(got_s != want_s)[:8]
    assert (got_r.astype(np.int64) == want_r).all(), np.flatnonzero(got_r != want_r)[:8]
    return want_r, want_s


# ------------------------------------------------------------------------------------- 1. random, three tiles, ragged
N1, T1, V1 = 2 * 4096 + 37, 4096, 300


@pytest.fixture(scope="module")
def case1(m, tmp_path_factory):
    D = rr.random_corpus(N1, V1, 24, seed=1)
    D[T1:, V1 - 1] = 0     # the last term has postings in tile 0 only (every doc keeps term 0: no empty rows)
    ix = rr.open_index(m, tmp_path_factory.mktemp("rank1") / "c1.idx", D, T1)
    light = rr.random_queries(64, 8, V1, seed=2)
    general = rr.random_queries(48, 90, V1, seed=3)
    n_l, dense = sparse_entries(ix.path, light)
    n_g, _ = sparse_entries(ix.path, general)
    assert ix.n_tiles == 3 and len(dense) >= 2 and 0 in dense      # default dense head; term 0 is the df == N term
    assert max(n_l) <= 64 and min(n_g) > 64                        # one batch per accumulation path
    yield dict(ix=ix, D=D, light=light, general=general, t_light=rr.random_targets(64, N1, seed=4),
               t_general=rr.random_targets(48, N1, seed=5))
    ix.close()


@pytest.mark.parametrize("drop", [True, False], ids=["drop_df_eq_n", "keep_df_eq_n"])
@pytest.mark.parametrize("path", ["light", "general"])
def test_random_three_ragged_tiles(case1, path, drop):
    c = case1
    t = c["t_" + path]
    assert any(len(x) == 0 for x in t) and any(len(set(x)) < len(x) for x in t)   # no targets / duplicates occur
    want_r, _ = check(c["ix"], c["D"], c[path], t, drop=drop)
    assert want_r.max() > 1024     # ranks beyond MSR_KMAX: what no search call can report


def test_ms_and_empty_calls(case1):
    c = case1
    q, t = rr.csr(c["light"]), rr.targets_csr(c["t_light"])
    r, s, ms = c["ix"].rank_docs(*q, *t, with_ms=True)
    assert ms[0] > 0 and ms[1] > 0
    r0, s0 = c["ix"].rank_docs(*q, np.zeros(65, np.int64), np.zeros(0, np.uint32))      # no target at all
    assert len(r0) == 0 and len(s0) == 0
    r1, _ = c["ix"].rank_docs(np.zeros(1, np.int64), [], [], np.zeros(1, np.int64), [])  # nq == 0
    assert len(r1) == 0


# ------------------------------------------------------------------------------------------------ 2. every tile size
@pytest.mark.parametrize("dense_max_terms", [16, 0], ids=["dense_head", "no_dense_head"])
@pytest.mark.parametrize("tile_docs", ar.TILE_SIZES)
def test_every_tile_size(m, tmp_path, tile_docs, dense_max_terms):
    n = tile_docs + 37
    D = rr.random_corpus(n, 96, 24, seed=tile_docs)
    with rr.open_index(m, tmp_path / "t.idx", D, tile_docs, dense_max_terms=dense_max_terms) as ix:
        light, general = rr.random_queries(16, 8, 96, seed=7), rr.random_queries(16, 90, 96, seed=8)
        n_l, dense = sparse_entries(ix.path, light)
        n_g, _ = sparse_entries(ix.path, general)
        assert ix.n_tiles == 2 and (len(dense) > 0) == (dense_max_terms > 0) and max(n_l) <= 64 and min(n_g) > 64
        rng = np.random.default_rng(9)
        for rows in (light, general):
            # 4 targets each: two random, one in the ragged tile, the tile's last accumulator
            tg = [rng.integers(0, n, size=2).tolist() + [int(rng.integers(tile_docs, n)), tile_docs - 1] for _ in rows]
            check(ix, D, rows, tg)


# ------------------------------------------------------------------------------------------------ 3. planted positions
def test_planted_positions(case1, m):
    c, D = case1, case1["D"]
    edges = [0, T1 - 1, T1, 2 * T1 - 1, 2 * T1, N1 - 1]    # first and last doc of each tile, last doc of the ragged one
    t_only0 = V1 - 1                           # (case1) postings in tile 0 only
    assert D[:T1, t_only0].any() and not D[T1:, t_only0].any()
    no_post_tile2 = [2 * T1 + 1, N1 - 2]       # targets in a tile where the query has no posting at all
    mx = m._cabi.MSR_RANK_MAX_TARGETS
    rows = [c["light"][0], c["general"][0], [(t_only0, 3)], [(0, 5), (-1, 2), (7, 0)], c["light"][1]]
    targets = [edges, edges, no_post_tile2 + edges, edges, list(range(T1 - mx // 2, T1 + mx // 2))]
    for drop in (True, False):
        want_r, want_s = check(c["ix"], D, rows, targets, drop=drop)
        tp = rr.targets_csr(targets)[0]
        assert (want_s[tp[2]:tp[2] + 2] == 0).all() and (want_r[tp[2]:tp[2] + 2] == 0).all()  # no posting: score 0, rank 0
        if drop:   # every term of query 3 is dropped (df == N, OOV, zero weight): every rank 0
            assert (want_r[tp[3]:tp[4]] == 0).all() and (want_s[tp[3]:tp[4]] == 0).all()
        assert tp[5] - tp[4] == mx
    check(c["ix"], D, rows[:1] + rows[2:], targets[:1] + targets[2:])     # the same on the light path alone


# ------------------------------------------------------------------------------------------------------ 4. mass ties
def test_mass_ties_across_a_tile_boundary(m, tmp_path):
    n = T1 + 700
    D = rr.random_corpus(n, 64, 12, seed=21)
    D[3800:4400] = D[3800]                       # 600 identical docs at ordinals 3800 .. 4399
    with rr.open_index(m, tmp_path / "ties.idx", D, T1) as ix:
        terms = np.flatnonzero(D[3800])[1:6]
        rows = [[(int(t), 3) for t in terms], [(int(t), 2) for t in terms] + [(int(t), 1) for t in range(20, 64)] * 2]
        assert sparse_entries(ix.path, rows)[0][1] > 64
        tg = [[3800, 4100, 4096, 4399, 4095]] * 2
        check(ix, D, rows[:1], tg[:1])                # the light accumulation
        want_r, want_s = check(ix, D, rows, tg)       # the general one, both queries
        for q in range(2):
            r = want_r[5 * q:5 * q + 5]
            assert len(set(want_s[5 * q:5 * q + 5])) == 1 and r[0] >= 1
            assert [r[1] - r[0], r[2] - r[0], r[3] - r[0], r[4] - r[0]] == [300, 296, 599, 295]   # ranks follow ordinals


# ------------------------------------------------------------------------------------------- 5. scores in [2^31, 2^32)
@pytest.mark.parametrize("variant,dmax,density", ar.top_variants(), ids=[v[0] for v in ar.top_variants()])
def test_scores_with_bit_31_set(m, tmp_path, variant, dmax, density):
    from mllm_sparse_retrieval_amd._cabi import MsrError

    p = ar.top_corpus(T1)
    path = ar.build(m, tmp_path / "top.idx", p, dmax, density)
    D = rr.doc_matrix(*p["docs"], p["n_terms"])
    names = list(ar.TOP_QUERIES)
    light = [ar.TOP_QUERIES[x] for x in names]
    general = light + [ar.TOP_GENERAL_EXTRA]
    rng = np.random.default_rng(3)
    fixed = [7, T1 + 3, 0, T1 - 1, T1, p["n_docs"] - 1, int(p["plateau"][0]), int(p["plateau"][-1])]
    with m.SparseIndex(path, device=0) as ix:
        assert ix.docid_table().tolist() == p["ids"]
        for rows in (light, general):
            tg = [fixed + rng.integers(0, p["n_docs"], size=8).tolist() for _ in rows]
            want_r, want_s = check(ix, D, rows, tg)
            assert want_s.max() == 0xFFFFFFFF and (want_s >= 2**31).sum() > len(want_s) // 2   # an unsigned comparison
            assert want_r.max() > 1024
        label, bad, err, ok = ar.TOP_REFUSALS[1]
        assert err == "OVERFLOW"
        with pytest.raises(MsrError) as e:
            ix.rank_docs(*rr.csr([ok, bad]), *rr.targets_csr([[7], [7]]))
        assert e.value.code == E_OVERFLOW


# --------------------------------------------------------------------------------------------------------- 6. self_ord
def test_self_ord(case1):
    c, D = case1, case1["D"]
    rows = c["light"][:12] + c["general"][:4]
    S = rr.scores(*rr.csr(rows), D)
    order = [np.lexsort((np.arange(N1), -S[q])) for q in range(len(rows))]
    tg, me = [], []
    for q in range(len(rows)):
        o = order[q]
        t = int(o[40])
        # self above the target, below it, equal to it, absent (-1)
        me.append([int(o[3]), int(o[300]), t, -1][q % 4])
        tg.append([t, int(o[0]), int(o[5000])])
    want_r, _ = check(c["ix"], D, rows, tg, self_ord=np.array(me, np.int32))
    assert [int(want_r[3 * q]) for q in range(4)] == [40, 41, 0, 41]
    check(c["ix"], D, rows, tg, self_ord=None)                    # a NULL self_ord array
    check(c["ix"], D, rows, tg, self_ord=np.full(len(rows), -1, np.int32))


def test_self_ord_tied_with_the_target(m, tmp_path):
    D = rr.random_corpus(T1 + 50, 40, 10, seed=33)
    D[[100, 4000, 4100]] = D[100]                # three docs with equal scores for every query, in two tiles
    with rr.open_index(m, tmp_path / "self.idx", D, T1) as ix:
        terms = np.flatnonzero(D[100])[1:5]
        rows = [[(int(t), 2) for t in terms]] * 4
        # target 4000: self tied on a lower ordinal (counted out), on a higher one (never counted), the target, none
        me = np.array([100, 4100, 4000, -1], np.int32)
        want_r, _ = check(ix, D, rows, [[4000, 100, 4100]] * 4, self_ord=me)
        base = int(want_r[9])
        assert [int(want_r[3 * q]) for q in range(4)] == [base - 1, base, 0, base]


# ----------------------------------------------------------------------------------------- 7. agreement with the search
@pytest.mark.parametrize("path", ["light", "general"])
def test_agreement_with_the_search(case1, path):
    c = case1
    q, tg = rr.csr(c[path]), c["t_" + path]
    tp, to = rr.targets_csr(tg)
    ranks, scores = c["ix"].rank_docs(*q, tp, to)
    for k in (1, 10, 1024):
        ords, _, u32, n = c["ix"].search_csr(*q, k)
        for qi in range(len(tg)):
            row = ords[qi, :n[qi]].tolist()
            for e in range(tp[qi], tp[qi + 1]):
                r, t = int(ranks[e]), int(to[e])
                assert (t in row) == (1 <= r <= k), (k, qi, t, r)
                if 1 <= r <= k:
                    assert row[r - 1] == t and u32[qi, r - 1] == scores[e]


# ------------------------------------------------------------------------------------------------------ 8. shard handles
def test_shard_handles_are_refused(case1, m):
    from mllm_sparse_retrieval_amd._cabi import MsrError

    q, t = rr.csr(case1["light"][:2]), rr.targets_csr([[1], [2]])
    for kw in (dict(shard=1, n_shards=3), dict(term_shard=(0, 2))):
        with m.SparseIndex(case1["ix"].path, device=0, **kw) as sh:
            with pytest.raises(MsrError) as e:
                sh.rank_docs(*q, *t)
            assert e.value.code == E_INVAL


# ---------------------------------------------------------------------------------------------------------- 10. passes
def test_query_split_of_the_count_phase(m, tmp_path):
    src = open(os.path.join(ROOT, "mllm_sparse_retrieval_amd", "csrc", "msr_device.hip")).read()
    per_pass = int(re.search(r"constexpr int kRankPassQueries = (\d+);", src).group(1))
    nq = per_pass + 1                                    # the last query is a pass of its own
    D = rr.random_corpus(T1 + 9, 48, 10, seed=41)
    uniq = rr.random_queries(64, 8, 48, seed=42) + [[(5, 7), (9, 1)]]
    tg_u = rr.random_targets(65, T1 + 9, seed=43, lo=1, hi=3)
    tg_u[64] = np.flatnonzero(D[:, 5])[[0, -1]].tolist()          # the lone query of the second pass has hits
    S = rr.scores(*rr.csr(uniq), D)
    wr, ws = rr.ranks(S, *rr.targets_csr(tg_u))
    tp_u = rr.targets_csr(tg_u)[0]
    which = np.concatenate([np.arange(nq - 1) % 64, [64]])
    rows, tg = [uniq[i] for i in which], [tg_u[i] for i in which]
    want_r = np.concatenate([wr[tp_u[i]:tp_u[i + 1]] for i in which])
    want_s = np.concatenate([ws[tp_u[i]:tp_u[i + 1]] for i in which])
    with rr.open_index(m, tmp_path / "split.idx", D, T1) as ix:
        got_r, got_s = ix.rank_docs(*rr.csr(rows), *rr.targets_csr(tg))
    assert (got_s == want_s).all() and (got_r == want_r).all()
    assert want_r[-len(tg_u[64]):].max() > 0


# ------------------------------------------------------------------------------------------------------------- 9. CLI
def test_cli_ranks(m, tmp_path, capsys):
    from mllm_sparse_retrieval_amd import cli

    out, runs = str(tmp_path / "enc"), str(tmp_path / "runs")
    cli.main(["encode", "--synthetic", "flickr", "--n_images", "1300", "--sparse_output_dir", out])
    lines = open(os.path.join(out, "query.tsv")).read().splitlines(True)[:300]
    q300 = str(tmp_path / "q300.tsv")
    open(q300, "w").writelines(lines)
    cli.main(["index", "--input", out])
    capsys.readouterr()
    cli.main(["search", "--sparse_index", out, "--depth", "1000", "--queries", q300, "--qrels",
              os.path.join(out, "qrels.csv"), "--ranks", "--save_dir", runs, "--quiet"])
    text = capsys.readouterr().out
    num = r"([0-9.e+-]+)"
    rec = re.search(r"Sparse reps recall: r@1 %s, r@5 %s, r@10 %s, r@100 %s, r@200 %s\n" % ((num,) * 5), text)
    rk = re.search(r"Sparse exact ranks: r@1 %s, r@5 %s, r@10 %s, r@100 %s, r@200 %s, mrr %s, medr %s, meanr %s, "
                   r"unranked (\d+), missing (\d+)\n" % ((num,) * 8), text)
    assert rec and rk, text
    assert [float(x) for x in rec.groups()] == [float(x) for x in rk.groups()[:5]]
    assert 0 < float(rk.group(1)) <= float(rk.group(5)) and rk.group(10) == "0" and float(rk.group(7)) >= 1
    rows = [ln.rstrip("\n").split("\t") for ln in open(os.path.join(runs, "sparse.ranks.tsv"))]
    assert len(rows) == 300 and [r[0] for r in rows] == [ln.split("\t")[0] for ln in lines]   # one target per caption
    pos = {}
    for ln in open(os.path.join(runs, "sparse.trec")):
        qid, _, docid, rank = ln.split()[:4]
        pos[qid, docid] = int(rank)
    inside = 0
    for qid, docid, rank, score in rows:
        assert docid == str(int(qid) // 5) and int(score) >= 0
        if 1 <= int(rank) <= 1000:
            assert pos[qid, docid] == int(rank)
            inside += 1
        else:
            assert (qid, docid) not in pos
    assert inside > 0
