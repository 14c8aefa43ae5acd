"""Inputs of the exact fusion tests (tests/test_fusion_ref.py on the CPU, tests/test_fusion_exact.py on the GPU), plain
numpy. A case holds everything a hybrid call takes and everything tests/fusion_ref.py needs:

    Dm       int64 [n_docs, n_terms]   doc weights by dense ROW (the CSR the index is built from: rank_ref.docs_to_csr)
    queries  [[(term, weight), ...]]   sparse queries
    p, q     f32 [n_docs, h], [nq, h]  dense rows and queries; prec = the handles they are exact on:
                 "fp16" entries are multiples of 1/8 in [-2, 2] and h <= 256 (every product a multiple of 1/64, every
                        partial sum below 2^10: f32 accumulation is exact in any order, tests/test_hybrid_union.py), so such
                        a case runs on BOTH handles;
                 "f32"  anything else: the k-ordered fmaf chain (tests/f32_chain.py), f32 handles only
    r2o      row -> ordinal, a seeded permutation (doc ids are the zero-padded ordinals): ordinal != row
    depth, alpha, self_ord, ks        the call; ks = the k values of the top-k entry points

scores(case) -> the exact sparse scores and the f32 dense scores of every doc BY ORDINAL, what fusion_ref.fuse takes.

planted() builds a case from the scores themselves: query i is one term of weight 1 whose doc weights are the wanted sparse
scores (<= 65535), and one dense coordinate: q_i = e_i, p[row, i] = the wanted dense score, which the fmaf chain and the
fp16 GEMM both return exactly."""
from __future__ import annotations

import functools

import numpy as np

from tests import rank_ref
from tests.f32_chain import chain_scores

N_SMALL, N_TWO_TILES, N_FIVE_TILES = 600, 4097, 4 * 4096 + 1   # one tile; 4096 + a last tile of ONE doc; 4 tiles + one doc


def _perm(n, seed):
    return np.random.default_rng(9000 + seed).permutation(n).astype(np.uint32)


def is_fp16_exact(x):
    x = np.asarray(x, dtype=np.float64)
    return bool((np.abs(x) <= 2).all() and (x * 8 == np.rint(x * 8)).all())


def make(name, Dm, queries, p, q, r2o, depth, alpha, self_ord=None, ks=(1, 10, 64, 65)):
    p, q = np.ascontiguousarray(p, dtype=np.float32), np.ascontiguousarray(q, dtype=np.float32)
    prec = "fp16" if is_fp16_exact(p) and is_fp16_exact(q) and p.shape[1] <= 256 else "f32"
    so = None if self_ord is None else np.asarray(self_ord, dtype=np.int32)
    return dict(name=name, Dm=np.asarray(Dm, dtype=np.int64), queries=queries, p=p, q=q, r2o=np.asarray(r2o, np.uint32),
                depth=int(depth), alpha=float(alpha), self_ord=so, ks=tuple(ks), prec=prec)


def planted(name, S, Dn, depth, alpha, self_ord=None, ks=(1, 10, 64, 65), seed=0):
    """S int [nq, n] and Dn f32 [nq, n]: the sparse and dense score of every doc BY ORDINAL."""
    S, Dn = np.asarray(S, dtype=np.int64), np.asarray(Dn, dtype=np.float32)
    nq, n = S.shape
    assert Dn.shape == (nq, n) and S.min() >= 0 and S.max() <= 65535
    assert ((S == 0).sum(axis=1) > 0).all(), "a term in every doc would be dropped (df == N)"
    r2o = _perm(n, seed)
    h = -(-nq // 8) * 8
    p, q = np.zeros((n, h), np.float32), np.zeros((nq, h), np.float32)
    p[:, :nq] = Dn.T[r2o]
    q[np.arange(nq), np.arange(nq)] = 1.0
    return make(name, S.T[r2o], [[(i, 1)] if S[i].any() else [] for i in range(nq)], p, q, r2o, depth, alpha, self_ord, ks)


def scores(case):
    """-> (S int64 [nq, n_docs], D float32 [nq, n_docs]) by ordinal."""
    qp, qt, qw = rank_ref.csr(case["queries"])
    s_row = rank_ref.scores(qp, qt, qw, case["Dm"])
    if case["prec"] == "fp16":
        d_row = case["q"] @ case["p"].T        # exact in f32 in any order (module docstring)
    else:
        d_row = chain_scores(case["q"], case["p"])
    r2o = case["r2o"].astype(np.int64)
    S, D = np.empty_like(s_row), np.empty_like(d_row)
    S[:, r2o], D[:, r2o] = s_row, d_row
    return S, D


# ------------------------------------------------------------------------------------------------ building blocks
def _eighths(rng, shape, lo=-16, hi=16):
    return (rng.integers(lo, hi + 1, shape) / 8.0).astype(np.float32)


def _base(n, nq, seed, hit=0.25, smax=500, dlo=-16, dhi=16):
    """Seeded background: a share `hit` of the docs with sparse scores 1..smax (the last doc never: df < N), dense scores
    multiples of 1/8 in [dlo / 8, dhi / 8] — a few dozen distinct values over hundreds of docs: exact dense ties everywhere,
    the depth boundary included."""
    rng = np.random.default_rng(100 + seed)
    S = rng.integers(1, smax + 1, (nq, n)) * (rng.random((nq, n)) < hit)
    S[:, -1] = 0
    return S.astype(np.int64), _eighths(rng, (nq, n), dlo, dhi), rng


# ------------------------------------------------------------------------------------------------ named edges
def mirror_tie(n):
    """alpha = 0.5: the best dense-only doc and the best sparse-only doc both score exactly 0.5 and every other member
    less (the two lists are disjoint, and nothing else reaches a list's maximum); k = 1 cuts between the two. Query 0:
    the dense doc has the lower ordinal, query 1: the sparse doc. Query 2: the pair sits on ordinals n - 2 / n - 1 (4095 /
    4096, the tile edge and the one-doc last tile, at n = 4097). The sparse list spans 1000 - 959 = 41, and
    41.0f * (1.0f / 41.0f) is NOT 1: only the exact 1 at the maximum keeps the tie a tie."""
    S, Dn, rng = _base(n, 3, 1, hit=0.1, dlo=-16, dhi=8)
    Dn[S > 0] = -2.0                                      # sparse hits far below the dense list: disjoint lists
    pairs = [(5, 17), (23, 11), (n - 2, n - 1)]           # (dense best, sparse best)
    for i, (a, b) in enumerate(pairs):
        rest = rng.choice(np.setdiff1d(np.arange(30, n - 2), np.flatnonzero(Dn[i] > 0.5)), 7, replace=False)
        S[i, rest], Dn[i, rest] = [995, 990, 985, 980, 975, 970, 959], -2.0
        S[i, a], Dn[i, a] = 0, 2.0
        S[i, b], Dn[i, b] = 1000, -2.0
    return planted("mirror_tie", S, Dn, 8, 0.5, ks=(1, 2, 64), seed=1)


def zero_weight(n, alpha):
    """alpha = 0 / 1: every member that only the zero-weight side holds sits at +0, the other side's last member too.
    depth 40 with nearly disjoint lists: k = 50 and 64 cut inside the block of zeros (one histogram bin of the
    single-tile kernel), by ordinal."""
    S, Dn, _ = _base(n, 4, 2, hit=0.2)
    return planted(f"zero_weight_{alpha:g}", S, Dn, 40, alpha, ks=(1, 50, 64, 65), seed=2)


def alpha_outside(n, alpha):
    """alpha = -0.25 / 1.5: one weight negative, fused scores of either sign; the order is still by the fused key."""
    S, Dn, _ = _base(n, 4, 3, hit=0.3)
    so = np.array([-1, 7, -1, n - 1], dtype=np.int32)
    return planted(f"alpha_{alpha:g}", S, Dn, 30, alpha, self_ord=so, ks=(1, 10, 64, 65), seed=3)


def depth_one(n):
    """depth = 1: max == min on both sides, every quotient is 0 / 1e-9: one or two members, all at +0."""
    S, Dn, _ = _base(n, 4, 4)
    S[1], Dn[1] = 0, Dn[0]
    S[1, 9] = 3
    Dn[1, 9] = 2.0                                        # query 1: the same doc heads both lists
    so = np.array([-1, -1, int(np.argmax(S[2])), -1], dtype=np.int32)
    return planted("depth_1", S, Dn, 1, 0.3, self_ord=so, ks=(1, 2, 64), seed=4)


def depth_ge_n():
    """depth >= n_docs (300 docs, depth 1024): the dense list is the whole corpus, the sparse list every hit."""
    S, Dn, _ = _base(300, 3, 5, hit=0.5)
    return planted("depth_ge_n", S, Dn, 1024, 0.3, self_ord=np.array([0, -1, 299], np.int32), ks=(1, 64, 65, 1024), seed=5)


def depth_1024(n):
    """depth = 1024, the largest: k = 1024 and a union of up to 2048."""
    S, Dn, _ = _base(n, 3, 6, hit=0.6, smax=60000)
    return planted("depth_1024", S, Dn, 1024, 0.3, self_ord=np.array([-1, 1, -1], np.int32), ks=(1, 64, 65, 1024), seed=6)


def short_lists(n):
    """A sparse list shorter than depth (query 0: five hits), an empty sparse query (1: no entry at all, the sparse side
    is {0, 0}), all sparse scores equal while the dense side has spread (2), all dense scores equal while the sparse side
    has spread (3: the dense list is decided by the dense tie rule alone), and both sides flat (4)."""
    S, Dn, rng = _base(n, 5, 7, hit=0.3)
    S[0] = 0
    S[0, [3, 50, 51, n - 2, 120]] = [9, 400, 400, 7, 1]
    S[1] = 0
    S[2] = np.where(S[2] > 0, 77, 0)
    Dn[3] = 0.625
    S[4] = np.where(S[4] > 0, 5, 0)
    Dn[4] = -1.5
    return planted("short_lists", S, Dn, 40, 0.3, ks=(1, 10, 64, 65), seed=7)


def self_extremes(n):
    """self_ord is the best / the last member of the dense list (queries 0, 1) and of the sparse list (2, 3): max and min
    still come from the unfiltered list, so no remaining member is at 1 (resp. at 0) on that side. Scores are distinct at
    both ends of both lists, so the removed doc IS the extreme. Query 4: self_ord heads both lists."""
    nq, depth = 5, 12
    S, Dn, rng = _base(n, nq, 8, hit=0.3, dlo=-4, dhi=4)             # dense background in [-0.5, 0.5]
    so = np.zeros(nq, dtype=np.int32)
    for i in range(nq):
        hits = np.flatnonzero(S[i])
        top_s = hits[np.argsort(-S[i, hits], kind="stable")][:depth]
        S[i, top_s] = 60000 - 37 * np.arange(depth)                  # the sparse list: all distinct
        top_d = rng.choice(n - 1, depth, replace=False)
        if i == 4:
            top_d = np.concatenate([[top_s[0]], top_d[top_d != top_s[0]]])[:depth]
        Dn[i, top_d] = 2.0 - np.arange(depth) / 8.0                  # the dense list: 2.0 ... 0.625, all distinct
        so[i] = [top_d[0], top_d[depth - 1], top_s[0], top_s[depth - 1], top_s[0]][i]
    return planted("self_extremes", S, Dn, depth, 0.3, self_ord=so, ks=(1, 10, 64), seed=8)


def dense_sign(n):
    """Dense scores all negative (queries 0, 1) and straddling zero with exact zeros among them (2, 3)."""
    S, Dn, rng = _base(n, 4, 9, hit=0.3)
    Dn[:2] = _eighths(rng, (2, n), -16, -1)
    Dn[2:] = _eighths(rng, (2, n), -3, 3)
    return planted("dense_sign", S, Dn, 50, 0.7, ks=(1, 10, 64, 65), seed=9)


def tile_edges(n):
    """The best docs of both lists on the last ordinals (n = 4097: 4095 and 4096, the last doc of the first tile and the
    only doc of the last one), in both assignments; query 2: the one-doc tile's doc is best on the dense side and self_ord."""
    S, Dn, _ = _base(n, 3, 10, hit=0.3, dhi=8)
    S[:, n - 1] = 0                                                   # (the last doc has no sparse hit: df < N)
    S[0, n - 2], Dn[0, n - 1] = 900, 2.0
    S[1, n - 2], Dn[1, n - 2], Dn[1, n - 1] = 900, 2.0, 1.875
    S[2, n - 2], Dn[2, n - 1] = 900, 2.0
    return planted("tile_edges", S, Dn, 25, 0.3, self_ord=np.array([-1, -1, n - 1], np.int32), ks=(1, 10, 64, 65), seed=10)


CARRIER = 65535


def large_sparse(n):
    """Sparse scores above 2^31, where an f32 holds every 256th integer (the top-of-range construction of
    tests/accum_ref.py: a carrier term of weight 65535 times a query weight). 200 docs hold the carrier (the sparse list is
    shorter than depth), a coarse term c in 0..41 that the query weighs 256 and a fine term f in 0..100 that it weighs 1:
    score = 65535 x 40048 + 256 c + f, and since 65535 x 40048 = 144 mod 256 every f below 240 rounds to the same f32:
    one image per c. Four docs have c = 41 (f = 100, 99, 98, 50): distinct u32 scores that share the image of the
    maximum, and one doc has c = 0, so the f32 spread is 41 x 256 — and 41.0f * (1.0f / 41.0f) is not 1: the three
    runners-up must NOT be given the maximum's exact 1, which only the comparison on the u32 score gets right.
    Query 1: the same, and self_ord is the doc that holds the maximum. Query 2 (carrier x 40000, fine term only): 101 u32
    scores, ONE f32 image: max == min in f32 and every sparse term is 0 / 1e-9 = 0 whatever the u32 scores say."""
    rng = np.random.default_rng(111)
    Dm = np.zeros((n, 3), dtype=np.int64)
    rows = rng.choice(n - 1, 200, replace=False)
    Dm[rows, 0] = CARRIER
    Dm[rows, 1] = rng.integers(1, 41, 200)
    Dm[rows, 2] = rng.integers(0, 101, 200)
    Dm[rows[:5], 1] = [41, 41, 41, 41, 0]
    Dm[rows[:4], 2] = [100, 99, 98, 50]
    r2o = _perm(n, 11)
    full = [(0, 40048), (1, 256), (2, 1)]
    queries = [full, full, [(0, 40000), (2, 1)]]
    p, q = np.zeros((n, 8), np.float32), np.zeros((3, 8), np.float32)
    p[:, :3] = _eighths(rng, (n, 3))
    q[np.arange(3), np.arange(3)] = 1.0
    so = np.array([-1, int(r2o[rows[0]]), -1], dtype=np.int32)
    return make("large_sparse", Dm, queries, p, q, r2o, 300, 0.3, self_ord=so, ks=(1, 10, 64, 65))


# ------------------------------------------------------------------------------------------------ random corpora
def random_case(prec, n, seed, nq=24, h=24, depth=300, alpha=0.3, ks=(1, 64, 65, 1024), dup_every=37):
    """A seeded corpus in the style of the neighbouring files: rank_ref.random_corpus / random_queries on the sparse side
    (two queries emptied / cut to one entry), normal f32 rows or 1/8-multiples on the dense side with every dup_every-th
    row a copy of row 0 (exact dense ties), remove_query on. alpha = 0.3: with 0.5 both weights are powers of two, every
    product is exact and a fused add could not be told from a separate multiply and add."""
    rng = np.random.default_rng(seed)
    Dm = rank_ref.random_corpus(n, 48, 10, seed)
    queries = rank_ref.random_queries(nq, 8, 48, seed + 1)
    queries[1], queries[2] = [], queries[2][:1]
    if prec == "fp16":
        p, q = _eighths(rng, (n, h)), _eighths(rng, (nq, h))
    else:
        p, q = rng.standard_normal((n, h)).astype(np.float32), rng.standard_normal((nq, h)).astype(np.float32)
    p[dup_every::dup_every] = p[0]
    r2o = _perm(n, seed)
    c = make(f"random_{prec}_{n}", Dm, queries, p, q, r2o, depth, alpha, self_ord=r2o[:nq].astype(np.int32), ks=ks)
    assert c["prec"] == prec
    return c


def fuzz_case(rng, n):
    """One draw of the seeded fuzz: planted scores with random density, score range, depth, alpha and self_ord."""
    nq = int(rng.integers(2, 7))
    S, Dn, _ = _base(n, nq, int(rng.integers(1 << 30)), hit=float(rng.choice([0.02, 0.3, 0.9])),
                     smax=int(rng.choice([3, 500, 65535])), dlo=int(rng.choice([-16, -2, 0])), dhi=int(rng.choice([0, 2, 16])))
    if rng.random() < 0.3:
        S[0] = 0
    depth = int(rng.choice([1, 2, 7, 64, 100, 1000, 1024]))
    alpha = float(rng.choice([0.0, 0.3, 0.5, 0.7, 1.0, -0.25, 1.5]))
    so = rng.integers(-1, n, nq).astype(np.int32) if rng.random() < 0.6 else None
    ks = tuple(int(x) for x in rng.choice([1, 2, 10, 64, 65, 200, 1024], 3, replace=False))
    return planted("fuzz", S, Dn, depth, alpha, self_ord=so, ks=ks, seed=int(rng.integers(1 << 30)))


EDGES = {
    "mirror_tie": mirror_tie, "zero_weight_0": lambda n: zero_weight(n, 0.0), "zero_weight_1": lambda n: zero_weight(n, 1.0),
    "alpha_-0.25": lambda n: alpha_outside(n, -0.25), "alpha_1.5": lambda n: alpha_outside(n, 1.5), "depth_1": depth_one,
    "depth_ge_n": lambda n: depth_ge_n(), "depth_1024": depth_1024, "short_lists": short_lists,
    "self_extremes": self_extremes, "dense_sign": dense_sign, "tile_edges": tile_edges, "large_sparse": large_sparse,
}
RANDOM = {"random_f32": lambda n: random_case("f32", n, 41), "random_fp16": lambda n: random_case("fp16", n, 42)}


@functools.lru_cache(maxsize=None)
def get(name, n):
    """The case and its per-ordinal scores, built once per (name, n) and shared (nothing may write to them)."""
    case = {**EDGES, **RANDOM}[name](n)
    S, D = scores(case)
    for a in (S, D, case["Dm"], case["p"], case["q"], case["r2o"]):
        a.setflags(write=False)
    return case, S, D
