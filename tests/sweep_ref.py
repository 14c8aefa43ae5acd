"""numpy reference for msr_hybrid_sweep (include/msr.h): slice a of a sweep is fusion_ref.topk(fusion_ref.fuse(S, D, depth,
alphas[a], self_ord), k), stacked per alpha. Nothing here calls libmsr; every comparison against it is exact equality.

A9 is the alpha grid of the sweep tests: both zero weights (0, 1), both out-of-range signs (-0.25, 1.5), and 0.3, where a
fused add differs from a rounded multiply and a rounded add (at 0.5 both weights are powers of two and every product is
exact).

full_union() plants the sort's capacity: depth 1024, 1024 sparse hits and the 1024 best dense docs disjoint, so every query
has exactly 2 x 1024 = 2048 members."""
from __future__ import annotations

import numpy as np

from tests import fusion_cases as fc
from tests import fusion_ref as fr

A9 = [0.0, 0.1, 0.3, 0.5, 0.7, 0.9, 1.0, -0.25, 1.5]
FULL_DEPTH = 1024
N_FULL_MIN = 2560     # docs full_union needs at least: 2048 members, background, one doc without a sparse hit


def sweep(S, D, depth, alphas, self_ord, k):
    """-> (ordinals uint32 [A, nq, k], score bits uint32 [A, nq, k], counts int32 [A, nq]), padded 0xFFFFFFFF / 0."""
    outs = [fr.topk(fr.fuse(S, D, depth, float(np.float32(a)), self_ord), k) for a in alphas]
    return tuple(np.stack([o[j] for o in outs]) for j in range(3))


def full_union(n, nq=3, seed=0):
    """-> (case, S, D): a planted case (fusion_cases.planted) of max(n, N_FULL_MIN) docs at depth 1024 whose every query has
    1024 sparse hits (all listed) and 1024 docs that beat every other doc on the dense side, the two sets disjoint: 2048
    members, the capacity of the sweep's sort. Sparse scores are distinct (1024 distinct fused scores at every alpha
    with w_s != 0), dense scores of the best 1024 are multiples of 1/8 in [0, 2] (17 values: fused ties among the
    dense-only members at every alpha, broken by ordinal); every other doc's dense score is in [-2, -1]. S and D are the
    planted scores by ordinal, which the f32 chain and the fp16 GEMM return exactly (fusion_cases.planted)."""
    n = max(int(n), N_FULL_MIN)
    rng = np.random.default_rng(7000 + seed)
    S = np.zeros((nq, n), dtype=np.int64)
    Dn = (rng.integers(-16, -7, (nq, n)) / 8.0).astype(np.float32)
    for i in range(nq):
        pick = rng.permutation(n - 1)[:2 * FULL_DEPTH]                  # (the last doc never: df < N)
        S[i, pick[:FULL_DEPTH]] = rng.permutation(65535)[:FULL_DEPTH] + 1
        Dn[i, pick[FULL_DEPTH:]] = (rng.integers(0, 17, FULL_DEPTH) / 8.0).astype(np.float32)
    case = fc.planted(f"full_union_{nq}", S, Dn, FULL_DEPTH, 0.3, ks=(1, 10, 65, 2 * FULL_DEPTH), seed=12 + seed)
    return case, S, Dn + np.float32(0.0)
