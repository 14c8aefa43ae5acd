"""tests/filter_ref.py against brute force, on the CPU: the bit layout of a doc set, the pack / unpack round trip (also
against the package's own packer), the masked top-k against a plain loop, the named sets."""
import numpy as np
import pytest

from tests import filter_ref as fr


def test_bit_layout_by_hand():
    member = np.zeros((2, 70), dtype=bool)
    member[0, [0, 31, 32, 69]] = True
    member[1, 33] = True
    w = fr.pack(member)
    assert w.dtype == np.uint32 and w.shape == (2, 3)
    assert w[0].tolist() == [0x80000001, 0x00000001, 1 << 5] and w[1].tolist() == [0, 2, 0]


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 4099, 8229])
def test_pack_unpack_round_trip(n):
    from mllm_sparse_retrieval_amd import filters

    rng = np.random.default_rng(n)
    member = rng.random((5, n)) < 0.4
    w = fr.pack(member)
    assert w.shape == (5, fr.words_of(n)) and (fr.unpack(w, n) == member).all()
    for s in range(5):                                                # brute force: one bit at a time
        for o in rng.integers(0, n, size=50):
            assert bool((int(w[s, o >> 5]) >> (o & 31)) & 1) == bool(member[s, o])
    assert (filters.pack_doc_sets(member) == w).all() and (filters.unpack_doc_sets(w, n) == member).all()
    assert (filters.sets_from_ordinals([np.flatnonzero(r) for r in member], n) == w).all()
    if n % 32:                                                        # garbage above n is ignored by unpack
        g = w.copy()
        g[:, -1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
        assert (fr.unpack(g, n) == member).all() and (filters.unpack_doc_sets(g, n) == member).all()


def test_masked_topk_against_a_loop():
    rng = np.random.default_rng(3)
    nq, n, k = 9, 57, 12
    K = rng.integers(0, 6, size=(nq, n))                              # small range: ties and zeros everywhere
    member = rng.random((3, n)) < 0.5
    member[2] = False
    q_set = np.array([-1, 0, 1, 2, 0, 1, -1, 2, 0])
    idx, keys, n_hit = fr.masked_topk(K, member, q_set, k)
    for i in range(nq):
        cand = [(int(K[i, c]), c) for c in range(n) if K[i, c] != 0 and (q_set[i] < 0 or member[q_set[i], c])]
        cand.sort(key=lambda t: (-t[0], t[1]))
        cand = cand[:k]
        assert n_hit[i] == len(cand)
        assert idx[i, :len(cand)].tolist() == [c for _, c in cand] and keys[i, :len(cand)].tolist() == [s for s, _ in cand]
        assert (idx[i, len(cand):] == 0xFFFFFFFF).all() and (keys[i, len(cand):] == 0).all()
    for kk in (1, 5, 12):
        for a, b in zip(fr.cut((idx, keys, n_hit), kk), fr.masked_topk(K, member, q_set, kk)):
            assert a.dtype == b.dtype and (a == b).all()
    # q_set None: one set for everyone / nothing filtered
    for a, b in zip(fr.masked_topk(K, member[:1], None, k), fr.masked_topk(K, member[:1], np.zeros(nq, int), k)):
        assert (a == b).all()
    for a, b in zip(fr.masked_topk(K, member[:0], None, k), fr.masked_topk(K, member, np.full(nq, -1), k)):
        assert (a == b).all()


def test_named_sets():
    n, tile = 2 * 4096 + 37, 4096
    member, words = fr.named_sets(n, tile)
    assert member.shape == (8, n) and words.shape == (8, fr.words_of(n)) and len(fr.SET_NAMES) == 8
    count = dict(zip(fr.SET_NAMES, member.sum(axis=1).tolist()))
    assert count["empty"] == 0 and count["full"] == count["full_garbage"] == n and count["last"] == 1
    assert count["tile1"] == tile and count["even"] == (n + 1) // 2 and count["span"] == tile - 2
    assert abs(count["random"] - n / 2) < 200
    assert (fr.unpack(words, n) == member).all()
    assert (words[:7] == fr.pack(member[:7])).all()
    assert words[7, -1] == 0xFFFFFFFF and words[1, -1] == (1 << (n % 32)) - 1    # the garbage is there
    assert not member[3, :tile].any() and not member[3, 2 * tile:].any()


def test_cut_rows_finds_a_planted_cut():
    K = np.array([[5, 3, 3, 3, 0, 1], [5, 4, 3, 2, 1, 0]])
    mask = np.ones_like(K, dtype=bool)
    assert fr.cut_rows(K, mask, 2) == [0] and fr.cut_rows(K, mask, 4) == []
    mask[0, 2] = False                                                # the class shrinks to two, k = 2 still cuts it
    assert fr.cut_rows(K, mask, 2) == [0] and fr.cut_rows(K, mask, 3) == []
