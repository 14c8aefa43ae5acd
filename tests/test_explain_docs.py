"""msr_explain_docs on the GPU against the numpy reference of tests/explain_ref.py (slot (e, j) = D[t, tau] when the entry
counts, else 0): exact equality of every slot, and the call's identity  sum_j max(omega_j, 0) * w(tau_j, t) == score
against ix.rank_docs on the same inputs — two walks over the index that share no kernel code. The shapes are the
smallest that reach each way explain_tiles (csrc/msr_explain.hpp) can go wrong: several tiles with a ragged last one,
every tile size with and without a dense head (both halves of a dense pair), padding postings that must never match a
listed doc, segment lengths around the 256-posting chunk edge, weights with bit 15 set, the target limit, queries
without entries, and the search path's and the CLI's own numbers."""
import functools
import json
import os
import shutil
from collections import Counter

import numpy as np
import pytest

from tests import accum_ref as ar
from tests import explain_ref as er
from tests import helpers
from tests import rank_ref as rr

pytestmark = pytest.mark.gpu

E_RANGE = -8
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sparse_small")


@pytest.fixture(scope="module")
def m(built):
    import mllm_sparse_retrieval_amd as m

    return m


def check(ix, D, rows, targets, drop=True):
    """Exact equality with the reference, then the identity against rank_docs. -> (x_ptr, doc_w, scores)."""
    q, t = rr.csr(rows), rr.targets_csr(targets)
    want_x, want_w = er.explain(*q, *t, D, drop)
    x, w = ix.explain_docs(*q, *t, drop_df_eq_n=drop)
    assert x.dtype == np.int64 and w.dtype == np.uint32
    assert (x == want_x).all() and len(w) == len(want_w)
    assert (w.astype(np.int64) == want_w).all(), np.flatnonzero(w != want_w)[:8]
    _, s = ix.rank_docs(*q, *t, drop_df_eq_n=drop)
    assert (er.row_scores(q[0], q[2], t[0], x, w) == s.astype(np.int64)).all()
    return x, w, s


# ------------------------------------------------------------------------------------- 1. random, three tiles, ragged
N1, T1, V1 = 2 * 4096 + 37, 4096, 300


@pytest.fixture(scope="module")
def case1(m, tmp_path_factory):
    D = rr.random_corpus(N1, V1, 24, seed=1)
    ix = rr.open_index(m, tmp_path_factory.mktemp("explain1") / "c1.idx", D, T1)
    f = helpers.read_index_file(ix.path)
    dense = {int(t) for t in f["dense_terms"] if t != ar.NO_TERM}
    assert ix.n_tiles == 3 and len(dense) >= 2 and 0 in dense      # default dense head; term 0 is the df == N term
    light = rr.random_queries(64, 8, V1, seed=2)       # each row: an OOV entry, q_w = 0, q_w < 0, a repeated term
    general = rr.random_queries(48, 90, V1, seed=3)
    for r in light + general:
        assert r[1][0] == -1 and r[2][1] == 0 and r[3][1] < 0 and r[4][0] == r[0][0]
    yield dict(ix=ix, D=D, light=light, general=general, t_light=rr.random_targets(64, N1, seed=4),
               t_general=rr.random_targets(48, N1, seed=5))
    ix.close()


@pytest.mark.parametrize("drop", [True, False], ids=["drop_df_eq_n", "keep_df_eq_n"])
@pytest.mark.parametrize("kind", ["light", "general"])
def test_random_three_ragged_tiles(case1, kind, drop):
    c = case1
    t = c["t_" + kind]
    assert any(len(x) == 0 for x in t) and any(len(set(x)) < len(x) for x in t)   # no targets / duplicates occur
    x, w, s = check(c["ix"], c["D"], c[kind], t, drop=drop)
    assert s.max() > 0 and np.count_nonzero(w) >= np.count_nonzero(s) > 0
    # a repeated term carries the same weight in both of its slots (slots 0 and 4 of every row)
    tp = rr.targets_csr(t)[0]
    for i in range(len(t)):
        for e in range(tp[i], tp[i + 1]):
            assert w[x[e]] == w[x[e] + 4]


def test_ms_and_empty_calls(case1):
    c = case1
    q, t = rr.csr(c["light"]), rr.targets_csr(c["t_light"])
    x, w, ms = c["ix"].explain_docs(*q, *t, with_ms=True)
    assert ms > 0
    x0, w0 = c["ix"].explain_docs(*q, np.zeros(65, np.int64), np.zeros(0, np.uint32))      # no target at all
    assert x0.tolist() == [0] and len(w0) == 0
    x1, w1 = c["ix"].explain_docs(np.zeros(1, np.int64), [], [], np.zeros(1, np.int64), [])  # nq == 0
    assert x1.tolist() == [0] and len(w1) == 0
    x2, w2 = c["ix"].explain_docs(np.zeros(3, np.int64), [], [], [0, 2, 3], [5, 9, 4100])    # only zero-length queries
    assert x2.tolist() == [0, 0, 0, 0] and len(w2) == 0


# ------------------------------------------------------------------------------------------------ 2. every tile size
@functools.lru_cache(maxsize=None)
def tile_corpus(tile_docs):
    n = tile_docs + 5
    D = rr.random_corpus(n, 96, 24, seed=tile_docs)
    tg = [0, tile_docs - 1, tile_docs, n - 1]      # local ordinal 0, tile - 1, first doc of the ragged tile, last doc
    D[tg, 1], D[tg, 2], D[tg, 3], D[tg, 4] = 7, 9, 0, 11   # head terms 1, 2, 4 present in every target, 3 absent
    D.setflags(write=False)
    return D, tg


@pytest.mark.parametrize("dense_max_terms", [16, 0], ids=["dense_head", "no_dense_head"])
@pytest.mark.parametrize("tile_docs", ar.TILE_SIZES)
def test_every_tile_size(m, tmp_path, tile_docs, dense_max_terms):
    D, tg = tile_corpus(tile_docs)
    with rr.open_index(m, tmp_path / "t.idx", D, tile_docs, dense_max_terms=dense_max_terms) as ix:
        f = helpers.read_index_file(ix.path)
        slot = {int(t): s for s, t in enumerate(f["dense_terms"]) if t != ar.NO_TERM}
        assert ix.n_tiles == 2 and (len(slot) > 0) == (dense_max_terms > 0)
        if dense_max_terms:
            assert set(slot) == {0, 1, 2, 3, 4}                       # the corpus' head: slots 0..4, both halves of a pair
            assert {slot[t] & 1 for t in (1, 2, 4)} == {0, 1}          # held terms on an even and on an odd slot
        hand = [(1, 3), (2, 4), (3, 5), (4, 6), (0, 2), (10, 2), (50, 3), (95, 1)]   # term 3: a head term the targets lack
        rows = [hand] + rr.random_queries(3, 8, 96, seed=7) + rr.random_queries(2, 90, 96, seed=8)
        for drop in (True, False):
            x, w, _ = check(ix, D, rows, [tg] * len(rows), drop=drop)
            for e in range(4):     # the hand-made query's rows
                assert w[x[e]:x[e] + 5].tolist() == [7, 9, 0, 11, 0 if drop else int(D[tg[e], 0])]


# --------------------------------------------------------------------------------------------- 3. padding cannot match
SEG_LENGTHS = [1, 5, 255, 256, 257, 513]     # postings of the planted terms 1..6 in tile 0


def test_padding_postings_never_match(m, tmp_path):
    n = T1 + 5
    D = np.zeros((n, 8), dtype=np.int64)
    D[:, 0] = 1                                               # every doc holds something
    planted = {}
    for t, L in enumerate(SEG_LENGTHS, start=1):
        docs = 1024 + np.arange(L) * 5 + t                    # local ordinals >= 1024, sorted: posting j is docs[j]
        assert docs.max() < T1
        D[docs, t] = 1 + (np.arange(L) * 7 + t) % 250
        planted[t] = docs
    with rr.open_index(m, tmp_path / "pad.idx", D, T1, dense_max_terms=0) as ix:
        f = helpers.read_index_file(ix.path)
        seg = f["seg_ptr"].astype(np.int64)
        post = f["postings"].reshape(-1, 4)
        pad_ords = set()
        for t, L in enumerate(SEG_LENGTHS, start=1):
            v = post[seg[0, t]:seg[0, t + 1]].ravel()
            assert np.count_nonzero(v >> 16) == L and len(v) == (L + 3) // 4 * 4
            pad_ords |= set((v[(v >> 16) == 0] & 0xFFFF).tolist())
        assert pad_ords and max(pad_ords) < 64        # the padding carries ordinals of docs 0..63, which hold no such term
        q_all = [(t, 3) for t in planted]
        edges = []
        for t, docs in planted.items():               # first / last posting, both sides of each 256-posting chunk edge
            edges += [int(docs[j]) for j in (0, len(docs) - 1, 255, 256, 511, 512) if j < len(docs)]
        assert len(edges) <= 64
        rows, tg = [q_all, q_all], [list(range(64)), edges]
        x, w, s = check(ix, D, rows, tg)
        assert not w[:x[64]].any() and not s[:64].any()           # docs 0..63: every slot 0
        got = w[x[64]:].reshape(len(edges), len(q_all))
        at = 0
        for t, docs in planted.items():
            for j in (0, len(docs) - 1, 255, 256, 511, 512):
                if j < len(docs):
                    assert got[at, t - 1] == 1 + (j * 7 + t) % 250 and np.count_nonzero(got[at]) == 1
                    at += 1


# ------------------------------------------------------------------------------------------------------- 4. weights
def test_weights_with_bit_15_set(m, tmp_path):
    n = T1 + 5
    D = np.zeros((n, 8), dtype=np.int64)
    D[:, 0] = 1
    weights = [1, 32767, 32768, 65535]
    ends = [0, T1 - 1]                                         # local ordinal 0 and tile - 1
    for t, wt in enumerate(weights, start=1):                  # sparse terms 1..4: one weight each, on both ends
        D[ends, t] = wt
    on = np.arange(n) % 5 != 2                                 # terms 5, 6: 80 % of the docs -> dense head, one pair
    D[on, 5] = np.where(np.arange(n)[on] % 2 == 0, 65535, 32768)
    D[on, 6] = np.where(np.arange(n)[on] % 2 == 0, 32768, 65535)
    assert on[0] and on[T1 - 1]
    with rr.open_index(m, tmp_path / "w.idx", D, T1) as ix:
        f = helpers.read_index_file(ix.path)
        slot = {int(t): s for s, t in enumerate(f["dense_terms"]) if t != ar.NO_TERM}
        assert {5, 6} <= set(slot) and {slot[5] & 1, slot[6] & 1} == {0, 1} and not {1, 2, 3, 4} & set(slot)
        rows = [[(4, 40000)], [(3, 70000)], [(2, 70000), (1, 5)], [(1, 16777215)], [(5, 30000), (6, 30000)],
                [(1, 9), (2, 9), (3, 9), (4, 40000), (5, 9), (6, 9)]]
        x, w, s = check(ix, D, rows, [ends + [1, T1]] * len(rows))
        assert (s.reshape(len(rows), 4)[[0, 1, 2, 4, 5], :2] >= 2**31).all()        # scores with bit 31 set
        assert w[x[0]] == 65535 and w[x[4]] == 32768 and w[x[8]] == 32767 and w[x[8] + 1] == 1
        assert sorted(w[x[16]:x[16] + 2].tolist()) == [32768, 65535]


# --------------------------------------------------------------------------------------------------------- 5. limits
def test_limits(case1, m):
    from mllm_sparse_retrieval_amd._cabi import MsrError

    c, D = case1, case1["D"]
    mx = m._cabi.MSR_EXPLAIN_MAX_TARGETS
    rng = np.random.default_rng(11)
    one = [(int(np.flatnonzero(D[T1 + 7])[3]), 6)]
    big = [(int(t), int(w)) for t, w in zip(rng.choice(V1, size=200, replace=False), rng.integers(1, 51, size=200))]
    full = list(range(T1 + 100, T1 + 100 + mx))                     # 64 distinct docs of one query in one tile
    rows = [c["light"][0], [], one, big, c["general"][0]]
    tg = [full, [3, N1 - 1], [T1 + 7, 0], [0, T1, N1 - 1], full[::-1]]
    x, w, s = check(c["ix"], D, rows, tg)
    tp = rr.targets_csr(tg)[0]
    assert x[tp[1]] == x[tp[2]] == mx * len(rows[0])                # the query without entries owns no slot
    assert w[x[tp[2]]] == D[T1 + 7, one[0][0]] > 0
    with pytest.raises(MsrError) as e:
        c["ix"].explain_docs(*rr.csr(rows[:1]), *rr.targets_csr([full + [T1 + 99]]))
    assert e.value.code == E_RANGE


# --------------------------------------------------------------------------------------------- 6. against the search
@pytest.mark.parametrize("kind", ["light", "general"])
def test_agreement_with_the_search(case1, kind):
    c = case1
    q = rr.csr(c[kind])
    ords, _, u32, n = c["ix"].search_csr(*q, 10)
    tg = [ords[i, :n[i]].tolist() for i in range(len(c[kind]))]
    tp, to = rr.targets_csr(tg)
    x, w = c["ix"].explain_docs(*q, tp, to)
    got = er.row_scores(q[0], q[2], tp, x, w)
    want = np.concatenate([u32[i, :n[i]] for i in range(len(tg))]).astype(np.int64)
    assert n.min() > 0 and (got == want).all()


# ------------------------------------------------------------------------------------------------------------- 7. CLI
def test_cli_explain(m, tmp_path, capsys):
    from mllm_sparse_retrieval_amd import cli

    work, runs = str(tmp_path / "enc"), str(tmp_path / "runs")
    shutil.copytree(GOLD, work)
    # ---- the expected text, from the corpus jsonl and the query file alone (whitespace-split keys, pieces add, weights
    # truncate toward zero and <= 0 is absent; tokens in every doc are dropped; score descending, doc id bytes ascending)
    docs = {}
    for line in open(os.path.join(work, "corpus_0.jsonl"), encoding="utf-8"):
        if line.strip():
            o = json.loads(line)
            vec = Counter()
            for key, val in o["vector"].items():
                if int(val) > 0:
                    for piece in key.split():
                        vec[piece] += int(val)
            docs[o["id"] if isinstance(o["id"], str) else json.dumps(o["id"])] = vec
    df = Counter(t for v in docs.values() for t in v)
    queries = [ln.rstrip("\n").split("\t") for ln in open(os.path.join(work, "query.tsv"), encoding="utf-8")]
    judged = {"1001": "1", "1002": "50", "1003": "7", "1004": "7", "1005": "3", "1006": "5", "9": "15", "1007": "8",
              "1008": "13", "1009": "11"}
    qrels = str(tmp_path / "qrels.csv")
    with open(qrels, "w") as f:
        f.write("imgid,filename,caption,sentid\n")
        f.writelines(f"{d},x.jpg,,{q}\n" for q, d in judged.items())
    want, shapes = [], set()
    for qid, text in queries:
        cnt = {t: c for t, c in Counter(text.split()).items() if df[t] != len(docs)}
        rows_of = {d: sorted(((t, c, v[t], c * v[t]) for t, c in cnt.items() if v.get(t, 0) > 0),
                             key=lambda r: (-r[3], r[0].encode())) for d, v in docs.items()}
        score = {d: sum(r[3] for r in rows_of[d]) for d in docs}
        hits = sorted((d for d in docs if score[d] > 0), key=lambda d: (-score[d], d.encode()))[:10]
        listed = hits[:3] + [d for d in [judged[qid]] if d not in hits[:3]]
        for d in listed:
            pos = hits.index(d) + 1 if d in hits else 0
            head = f"{qid}\t{d}\t{pos}\t{int(d == judged[qid])}\t{score[d]}"
            shapes.add((pos > 3, pos == 0, score[d] == 0, d == judged[qid]))
            want += [f"{head}\t{t}\t{c}\t{w}\t{x}\n" for t, c, w, x in rows_of[d]] or [head + "\t-\t0\t0\t0\n"]
    # the fixture reaches: a judged doc among the first 3 hits, one returned below them, one scored but cut by the
    # depth, one with score 0
    assert {(False, False, False, True), (True, False, False, True), (False, True, False, True),
            (False, True, True, True)} <= shapes
    cli.main(["index", "--input", work])
    capsys.readouterr()
    cli.main(["search", "--sparse_index", work, "--depth", "10", "--explain", "3", "--qrels", qrels, "--save_dir", runs,
              "--quiet"])
    out = capsys.readouterr().out
    text = open(os.path.join(runs, "sparse.explain.tsv"), encoding="utf-8").read()
    assert text == "".join(want)
    n_pairs = len({tuple(ln.split("\t")[:2]) for ln in want})
    assert f"Sparse explain: {n_pairs} (query, doc) pairs" in out
    with pytest.raises(SystemExit) as e:
        cli.main(["search", "--sparse_index", work, "--passage_reps", work, "--explain", "3"])
    assert isinstance(e.value.code, str) and "--explain" in e.value.code and "--passage_reps" in e.value.code
