"""numpy reference for the hybrid fusion contract of include/msr.h (msr_hybrid_search): both depth lists, the fused score
of every member of their union as f32 BITS, and the fully ordered union. Plain numpy float32 operations plus
tests/f32_chain.fmaf; nothing here calls libmsr, and every comparison against it is exact equality.

    w_d = (float)alpha, w_s = 1.0f - w_d
    per side: max / min = the best and the last score of the UNFILTERED depth list (sparse: (float)u32; dense: -0 -> +0;
              an empty list: 0, 0), inv = 1.0f / fmaxf(max - min, 1e-9f)
    t(x)  = 1.0f when x is the list's maximum and max > min (sparse: compared on the exact u32 score),
            else (x - min) * inv                       one rounded subtraction, one rounded multiplication
    f     = +0.0f;  f = fmaf(w_d, t_d, f) if the dense list holds the doc;  f = fmaf(w_s, t_s, f) if the sparse one does
    members = union of the two lists minus self_ord, by (fused key descending, ordinal ascending); the first k returned

Two entry points: fuse() from the per-ordinal scores of both sides, refuse_union() from the outputs of one
msr_hybrid_search_union call (arithmetic and order on inputs whose dense scores have no exact CPU reference).

CONTRACT is the arithmetic above; the other Variant fields switch one rule each to what a subtly wrong kernel would
compute (tests/test_fusion_ref.py counts how many members each of them moves)."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from tests.f32_chain import f32_keys, fmaf

PAD = 0xFFFFFFFF
F1, F0 = np.float32(1.0), np.float32(0.0)
EPS = np.float32(1e-9)

# recip: (x - min) * (1 / den) instead of (x - min) / den;  exact_one: exactly 1 at the maximum;  fused_add: fmaf
# instead of a rounded product and a rounded sum;  u32_cmp: the sparse maximum found on the u32 score, not on its f32
# image;  unfiltered: max / min from the lists BEFORE self_ord is taken out
Variant = namedtuple("Variant", "recip exact_one fused_add u32_cmp unfiltered", defaults=(True,) * 5)
CONTRACT = Variant()

# One batch, laid out like msr_hybrid_search_union's outputs ([nq][2 x depth], padded the same way; bits = the f32 bit
# patterns of out_score), plus both depth lists per query as (ordinals, scores) best first
Fused = namedtuple("Fused", "ords bits cnt src su de rng s_lists d_lists")


def weights(alpha):
    w_d = np.float32(alpha)
    return w_d, np.float32(F1 - w_d)


def u32_to_f32(x):
    """(float)u32, round to nearest even (numpy converts int64 -> float32 by the same rule; 2^32, the image of the
    largest scores, is accepted so that an f32 extreme can be handed back as an integer)."""
    return np.asarray(x, dtype=np.int64).astype(np.float32)


def fused_scores(in_d, in_s, su, de, dmax, dmin, smax_u, smin_u, alpha, v=CONTRACT):
    """Fused f32 scores of members given elementwise: in_d / in_s (bool), su (exact sparse scores, integers), de (f32
    dense scores); dmax / dmin (f32) and smax_u / smin_u (integers, 0 for an empty list) scalars of the query."""
    w_d, w_s = weights(alpha)
    de = np.asarray(de, dtype=np.float32) + F0
    su = np.asarray(su, dtype=np.int64)
    dmax, dmin = np.float32(dmax) + F0, np.float32(dmin) + F0
    smax, smin = u32_to_f32(smax_u), u32_to_f32(smin_u)
    x_s = u32_to_f32(su)
    den_d, den_s = np.maximum(np.float32(dmax - dmin), EPS), np.maximum(np.float32(smax - smin), EPS)
    if v.recip:
        t_d, t_s = (de - dmin) * np.float32(F1 / den_d), (x_s - smin) * np.float32(F1 / den_s)
    else:
        t_d, t_s = (de - dmin) / den_d, (x_s - smin) / den_s
    if v.exact_one:
        s_at_max = (su == int(smax_u)) if v.u32_cmp else (x_s == smax)
        t_d = np.where((de == dmax) & bool(dmax > dmin), F1, t_d)
        t_s = np.where(s_at_max & bool(smax > smin), F1, t_s)
    t_d, t_s = t_d.astype(np.float32), t_s.astype(np.float32)
    f = np.zeros(len(su), dtype=np.float32)
    if v.fused_add:
        f = np.where(in_d, fmaf(w_d, t_d, f), f)
        f = np.where(in_s, fmaf(w_s, t_s, f), f)
    else:
        f = np.where(in_d, f + w_d * t_d, f).astype(np.float32)
        f = np.where(in_s, f + w_s * t_s, f).astype(np.float32)
    return f.astype(np.float32)


def fused_order(ords, f):
    """Positions of the members by (fused key descending, ordinal ascending)."""
    return np.lexsort((np.asarray(ords, dtype=np.int64), -f32_keys(f).astype(np.int64)))


def depth_lists(s_row, d_row, depth, tie):
    """Both depth lists of one query, ordinals best first. s_row: exact sparse score per ordinal (0 = no hit, never
    listed; ties to the lower ordinal); d_row: f32 dense score per ordinal (every doc is a hit; ties to the lower
    tie[ordinal])."""
    s_row = np.asarray(s_row, dtype=np.int64)
    hit = np.flatnonzero(s_row > 0)
    s_ord = hit[np.lexsort((hit, -s_row[hit]))][:depth]
    d_ord = np.lexsort((np.asarray(tie, dtype=np.int64), -f32_keys(d_row).astype(np.int64)))[:depth]
    return s_ord, d_ord


def fuse(S, D, depth, alpha, self_ord=None, row2ord=None, v=CONTRACT):
    """S: exact sparse scores int [nq, n_docs] by ORDINAL (rank_ref.scores); D: f32 dense scores [nq, n_docs] by ordinal;
    self_ord: [nq] ordinal to leave out or -1, or None; row2ord: None = dense ties to the lower ordinal (the candidate
    paths), else the dense row -> ordinal map = dense ties to the lower ROW (the list path). -> Fused."""
    S = np.asarray(S, dtype=np.int64)
    D = np.asarray(D, dtype=np.float32) + F0
    nq, n = S.shape
    assert D.shape == (nq, n) and S.min(initial=0) >= 0 and S.max(initial=0) <= 0xFFFFFFFF
    tie = np.arange(n)
    if row2ord is not None:
        tie = np.empty(n, dtype=np.int64)
        tie[np.asarray(row2ord, dtype=np.int64)] = np.arange(n)      # the row of every ordinal
    w = 2 * depth
    out = Fused(np.full((nq, w), PAD, np.uint32), np.zeros((nq, w), np.uint32), np.zeros(nq, np.int32),
                np.zeros((nq, w), np.uint8), np.zeros((nq, w), np.uint32), np.zeros((nq, w), np.float32),
                np.zeros((nq, 4), np.float32), [], [])
    for i in range(nq):
        me = -1 if self_ord is None else int(self_ord[i])
        s_ord, d_ord = depth_lists(S[i], D[i], depth, tie)
        out.s_lists.append((s_ord, S[i, s_ord]))
        out.d_lists.append((d_ord, D[i, d_ord]))
        s_rng, d_rng = (s_ord, d_ord) if v.unfiltered else (s_ord[s_ord != me], d_ord[d_ord != me])
        smax_u, smin_u = (int(S[i, s_rng[0]]), int(S[i, s_rng[-1]])) if len(s_rng) else (0, 0)
        dmax, dmin = (D[i, d_rng[0]], D[i, d_rng[-1]]) if len(d_rng) else (F0, F0)
        out.rng[i] = [dmax, dmin, u32_to_f32(smax_u), u32_to_f32(smin_u)]
        mem = np.union1d(s_ord, d_ord)
        mem = mem[mem != me]
        in_d, in_s = np.isin(mem, d_ord), np.isin(mem, s_ord)
        f = fused_scores(in_d, in_s, S[i, mem], D[i, mem], dmax, dmin, smax_u, smin_u, alpha, v)
        o = fused_order(mem, f)
        c = len(mem)
        out.cnt[i] = c
        out.ords[i, :c] = mem[o]
        out.bits[i, :c] = f[o].view(np.uint32)
        out.src[i, :c] = (in_d.astype(np.uint8) | (in_s.astype(np.uint8) << 1))[o]
        out.su[i, :c] = np.where(in_s, S[i, mem], 0)[o]
        out.de[i, :c] = np.where(in_d, D[i, mem], F0)[o]
    return out


def topk(fused, k):
    """What msr_hybrid_search[_f32] returns for k: (ordinals [nq, k], score bits [nq, k], counts), padded PAD / 0."""
    nq, w = fused.ords.shape
    ords, bits = np.full((nq, k), PAD, np.uint32), np.zeros((nq, k), np.uint32)
    cnt = np.minimum(fused.cnt, k).astype(np.int32)
    for i in range(nq):
        ords[i, :cnt[i]] = fused.ords[i, :cnt[i]]
        bits[i, :cnt[i]] = fused.bits[i, :cnt[i]]
    return ords, bits, cnt


def refuse_union(ords, cnt, src, su, de, rng, alpha, smax_u=None, v=CONTRACT):
    """The fused scores and the order recomputed from one union call's OWN outputs (out_ord, out_n, out_src,
    out_sparse_u32, out_dense, out_range) -> (ordinals, score bits) in the layout and padding of out_ord / out_score.
    The exact sparse maximum is not among the outputs: it is taken to be the best sparse member's score when that has the
    f32 image out_range reports, and to be held by no member otherwise (self_ord was the only best). Scores of 2^24 and
    more can share that image with a smaller one: pass smax_u ([nq]) where self_ord may have been the best of such a list."""
    ords, su = np.asarray(ords), np.asarray(su)
    out_o, out_b = np.full(ords.shape, PAD, np.uint32), np.zeros(ords.shape, np.uint32)
    for i in range(len(cnt)):
        c = int(cnt[i])
        in_d, in_s = (src[i, :c] & 1) != 0, (src[i, :c] & 2) != 0
        dmax, dmin, smax, smin = np.asarray(rng[i], dtype=np.float32)
        assert smax == np.rint(smax) and smin == np.rint(smin) and 0 <= smin <= smax <= 2.0**32
        if smax_u is not None:
            top = int(smax_u[i])
        else:
            best = int(su[i, :c][in_s].max(initial=0))
            top = best if u32_to_f32(best) == smax else -1
        # (fused_scores takes the extremes as integers: smin's image is exact for itself, and the maximum is given as an
        # integer with the reported image, or as that image when no member holds it)
        f = fused_scores(in_d, in_s, su[i, :c], de[i, :c], dmax, dmin, top if top >= 0 else int(smax), int(smin), alpha, v)
        o = fused_order(ords[i, :c], f)
        out_o[i, :c] = ords[i, :c][o]
        out_b[i, :c] = f[o].view(np.uint32)
    return out_o, out_b
