"""tests/hybrid_filter_ref.py on the CPU: the sub-corpus reference of filtered deep hybrid search (fusion_ref.fuse on the
columns of a query's set, ordinals mapped back) against a second, independent formulation: tests/fuse_rows_ref.fuse_rows /
select on the MASKED rows S * member and f32_keys(D + 0) * member, which is what msr_hybrid_deep_filtered runs on the
device. Every comparison is exact equality: ordinals, score bits, counts, members, sources, extremes, both depth lists."""
import numpy as np
import pytest

from tests import fuse_rows_ref as rr
from tests import fusion_ref as fr
from tests import hybrid_filter_ref as hf
from tests.f32_chain import f32_keys
from tests.test_fuse_rows_ref import DEPTH, N_DEEP, deep_corpus


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("alpha", [0.3, 1.5])
@pytest.mark.parametrize("depth", [1, 100, DEPTH, N_DEEP])
def test_sub_corpus_equals_masked_rows(depth, alpha):
    S, D, so = deep_corpus()
    nq, n = S.shape
    member = hf.standard_sets(n, DEPTH)
    K = f32_keys(D + fr.F0)
    k = min(2 * depth, n)
    for s, name in enumerate(hf.SET_NAMES):
        want = hf.fuse(S, D, member, np.full(nq, s), depth, alpha, so)
        rows = rr.fuse_rows(S * member[s], K * member[s].astype(np.uint32), depth, alpha, so)
        what = (name, depth, alpha)
        assert (rows.members == want.cnt).all(), what
        assert (rows.rng.view(np.uint32) == want.rng.view(np.uint32)).all(), what
        assert (rows.F[:, ~member[s]] == 0).all() and (rows.src[:, ~member[s]] == 0).all(), what
        for i in range(nq):
            assert (rows.s_lists[i][0] == want.s_lists[i][0]).all() and (rows.s_lists[i][1] == want.s_lists[i][1]).all(), what
            assert (rows.d_lists[i][0] == want.d_lists[i][0]).all(), what
            assert (_bits(rows.d_lists[i][1]) == _bits(want.d_lists[i][1])).all(), what
        o, b, c, src = rr.select(rows, k)
        assert (c == np.minimum(want.cnt, k)).all(), what
        assert (o == want.ords[:, :k]).all() and (b == want.bits[:, :k]).all() and (src == want.src[:, :k]).all(), what
        wo, wb, wc = fr.topk(want, 1)
        o, b, c, _ = rr.select(rows, 1)
        assert (o == wo).all() and (b == wb).all() and (c == wc).all(), what


def test_full_set_and_unfiltered_are_the_unfiltered_reference():
    S, D, so = deep_corpus()
    member = hf.standard_sets(S.shape[1], DEPTH)
    want = fr.fuse(S, D, DEPTH, 0.3, so)
    for q_set in (np.zeros(8, int), np.full(8, -1)):
        got = hf.fuse(S, D, member, q_set, DEPTH, 0.3, so)
        for a, b in zip(got[:7], want[:7]):
            assert (np.asarray(a).view(np.uint32) == np.asarray(b).view(np.uint32)).all() if a.dtype == np.float32 else (a == b).all()
        for i in range(8):
            assert (got.s_lists[i][0] == want.s_lists[i][0]).all() and (got.d_lists[i][0] == want.d_lists[i][0]).all()


def test_empty_set_gives_nothing_and_the_sets_are_what_they_say():
    S, D, so = deep_corpus()
    n = S.shape[1]
    member = hf.standard_sets(n, DEPTH)
    assert member.sum(axis=1).tolist()[:6] == [n, 0, 1, n - 8192, DEPTH, DEPTH + 1]
    assert 0.45 * n < member[6].sum() < 0.55 * n and 0.07 * n < member[7].sum() < 0.13 * n
    got = hf.fuse(S, D, member, np.full(8, 1), DEPTH, 0.3, so)
    assert (got.cnt == 0).all() and (got.ords == fr.PAD).all() and (got.bits == 0).all() and (got.rng == 0).all()
    assert all(len(x[0]) == 0 for x in got.s_lists + got.d_lists)
    # a self_ord outside the set changes nothing; inside, it leaves the union but stays in the lists and the extremes
    two = np.stack([member[6], ~member[6]])
    for s_i in (0, 1):
        q_set = np.full(8, s_i)
        inside = (so >= 0) & two[s_i][np.maximum(so, 0)]
        assert inside.any() == (s_i == 0) and ((so >= 0) & ~inside).any() == (s_i == 1)   # (the four self_ords: all in the half)
        a = hf.fuse(S, D, two, q_set, DEPTH, 0.3, so)
        c = hf.fuse(S, D, two, q_set, DEPTH, 0.3, None)
        for i in range(8):
            assert (a.rng[i] == c.rng[i]).all() and (a.d_lists[i][0] == c.d_lists[i][0]).all()
            if inside[i]:
                assert so[i] in c.ords[i] and so[i] not in a.ords[i] and a.cnt[i] == c.cnt[i] - 1
            else:
                assert (a.ords[i] == c.ords[i]).all() and (a.bits[i] == c.bits[i]).all() and a.cnt[i] == c.cnt[i]
