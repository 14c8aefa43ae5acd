"""tests/fusion_ref.py, the exact f32 reference of the hybrid fusion contract (include/msr.h, msr_hybrid_search), on the
CPU: hand-computed cases, agreement with the float64 oracle.fuse (the project's semantic anchor) on the inputs of
tests/test_fusion_exact.py, and the discriminating power of those inputs: how many members of their unions change bits when
ONE rule of the contract is replaced by what a subtly wrong kernel would compute."""
import numpy as np
import pytest

from tests import fusion_cases as fc
from tests import fusion_ref as fr
from tests import helpers

ALL = [(name, n) for name in list(fc.EDGES) + list(fc.RANDOM) for n in (fc.N_SMALL, fc.N_TWO_TILES)] + \
      [(name, fc.N_FIVE_TILES) for name in fc.RANDOM]


def f32(x):
    return np.float32(x)


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------- hand-computed cases
def test_hand_computed_small():
    """5 docs, depth 3, alpha = 0.25. Dense list: docs 0, 1, 2 with 3, 2, 1: inv = 1 / 2, t = 1, 0.5, 0. Sparse list: docs
    2, 3, 4 with 9, 5, 1: inv = 1 / 8, t = 1, 0.5, 0. Every product is exact: fused = 0.25, 0.125, 0 + 0.75, 0.375, 0."""
    S = np.array([[0, 0, 9, 5, 1]])
    D = np.array([[3, 2, 1, 0.5, -7]], dtype=np.float32)
    r = fr.fuse(S, D, 3, 0.25)
    assert r.cnt.tolist() == [5] and r.ords[0, :5].tolist() == [2, 3, 0, 1, 4]
    assert (r.bits[0, :5] == bits([0.75, 0.375, 0.25, 0.125, 0.0])).all() and (r.bits[0, 5:] == 0).all()
    assert r.src[0, :5].tolist() == [3, 2, 1, 1, 2] and (r.ords[0, 5:] == fr.PAD).all()
    assert r.su[0].tolist() == [9, 5, 0, 0, 1, 0] and r.de[0].tolist() == [1, 0, 3, 2, 0, 0]
    assert r.rng[0].tolist() == [3, 1, 9, 1]
    assert [x.tolist() for x in r.s_lists[0]] == [[2, 3, 4], [9, 5, 1]] and r.d_lists[0][0].tolist() == [0, 1, 2]
    o, b, c = fr.topk(r, 2)
    assert o.tolist() == [[2, 3]] and (b == bits([[0.75, 0.375]])).all() and c.tolist() == [2]
    o, b, c = fr.topk(r, 8)
    assert c.tolist() == [5] and (o[0, 5:] == fr.PAD).all() and (b[0, 5:] == 0).all()
    # self_ord = the best doc of BOTH sides' extremes: max and min stay those of the unfiltered lists
    r = fr.fuse(S, D, 3, 0.25, self_ord=[2])
    assert r.ords[0, :4].tolist() == [3, 0, 1, 4] and (r.bits[0, :4] == bits([0.375, 0.25, 0.125, 0.0])).all()
    assert r.rng[0].tolist() == [3, 1, 9, 1]
    # a doc in both lists with two inexact products: fmaf twice, by hand in float64 (both sums are exact there)
    S = np.array([[0, 7, 9, 5, 1]])
    r = fr.fuse(S, D, 3, 0.3)
    w_d, w_s = f32(0.3), f32(1) - f32(0.3)
    t_d, t_s = f32(f32(2 - 1) * f32(0.5)), f32(f32(7 - 5) * (f32(1) / f32(4)))
    first = f32(float(w_d) * float(t_d))
    want = f32(float(w_s) * float(t_s) + float(first))
    i = r.ords[0].tolist().index(1)
    assert r.src[0, i] == 3 and r.bits[0, i] == bits(want)


def test_mirror_tie_at_exactly_one_half():
    """alpha = 0.5: the best dense-only doc and the best sparse-only doc tie at EXACTLY 0.5 although 41.0f * (1.0f / 41.0f)
    is not 1, and the tie goes to the lower ordinal."""
    assert f32(41) * (f32(1) / f32(41)) != f32(1)
    for n in (fc.N_SMALL, fc.N_TWO_TILES):
        case, S, D = fc.get("mirror_tie", n)
        r = fr.fuse(S, D, case["depth"], case["alpha"])
        assert (r.bits[:, :2] == bits(0.5)).all() and (r.bits[:, 2] < bits(0.5)).all()
        assert r.ords[:, :2].tolist() == [[5, 17], [11, 23], [n - 2, n - 1]]
        assert r.src[:, :2].tolist() == [[1, 2], [2, 1], [1, 2]]
        assert (r.rng[:, 2] - r.rng[:, 3] == 41).all()
        wrong = fr.fuse(S, D, case["depth"], case["alpha"], v=fr.Variant(exact_one=False))
        assert (wrong.bits[:, 1] != bits(0.5)).all() and wrong.ords[1, 0] == 23   # the tie is gone, query 1 flips


def test_flat_and_empty_lists():
    """max == min: every quotient is 0 / 1e-9 = 0, never 1. An empty list: range {0, 0}, no term."""
    S = np.array([[4, 4, 4, 0, 0, 0], [0, 0, 0, 0, 0, 0]])
    D = np.array([[1, 1, 1, 1, 1, 1], [5, 4, 3, 2, 1, 0]], dtype=np.float32)
    r = fr.fuse(S, D, 3, 0.3)
    assert r.cnt.tolist() == [3, 3] and r.ords[:, :3].tolist() == [[0, 1, 2], [0, 1, 2]]
    assert (r.bits[0] == 0).all() and r.src[0, :3].tolist() == [3, 3, 3] and r.rng[0].tolist() == [1, 1, 4, 4]
    assert r.rng[1].tolist() == [5, 3, 0, 0] and r.src[1, :3].tolist() == [1, 1, 1]
    assert (r.bits[1, :3] == bits([f32(0.3), f32(f32(0.3) * f32(0.5)), 0])).all()
    # dense ties at the depth boundary: to the lower ordinal, or to the lower ROW when a row map is given
    r2o = np.array([5, 4, 3, 2, 1, 0])
    assert fr.fuse(S, D, 3, 0.3, row2ord=r2o).d_lists[0][0].tolist() == [5, 4, 3]
    assert fr.fuse(S, D, 3, 0.3).d_lists[0][0].tolist() == [0, 1, 2]


def test_large_sparse_case_is_what_it_says():
    for n in (fc.N_SMALL, fc.N_TWO_TILES):
        case, S, D = fc.get("large_sparse", n)
        r = fr.fuse(S, D, case["depth"], case["alpha"], case["self_ord"])
        assert all(len(s[0]) == 200 < case["depth"] and s[1].min() > 2**31 for s in r.s_lists)
        top = r.s_lists[0][1]
        shared = top[fr.u32_to_f32(top) == fr.u32_to_f32(top[0])]
        assert len(shared) == 4 and len(set(shared.tolist())) == 4                  # four u32 scores, one f32 image
        assert r.rng[0, 2] - r.rng[0, 3] == 41 * 256 and case["self_ord"][1] == r.s_lists[1][0][0]
        flat = r.s_lists[2][1]
        assert len(set(flat.tolist())) > 50 and len(set(fr.u32_to_f32(flat).tolist())) == 1 and r.rng[2, 2] == r.rng[2, 3]
        # members that hold the maximum's image but not the maximum sit just below the exact 1 of the maximum
        i = r.su[0].tolist().index(int(top[1]))
        j = r.su[0].tolist().index(int(top[0]))
        t_max, t_next = fr.fused_scores([False] * 2, [True] * 2, top[:2], [0, 0], 0, 0, top[0], top[-1], 0.0)
        assert t_max == 1 and t_next < 1 and r.src[0, i] & 2 and r.src[0, j] & 2


def test_refuse_union_reproduces_fuse():
    """The second entry point, fed the reference's own union, returns it unchanged (smax_u given where self_ord removed the
    only holder of a maximum above 2^24: fusion_ref.refuse_union)."""
    for name, n in ALL:
        case, S, D = fc.get(name, n)
        r = fr.fuse(S, D, case["depth"], case["alpha"], case["self_ord"])
        smax_u = [int(s[1][0]) if len(s[1]) else 0 for s in r.s_lists] if name == "large_sparse" else None
        o, b = fr.refuse_union(r.ords, r.cnt, r.src, r.su, r.de, r.rng, case["alpha"], smax_u=smax_u)
        assert (o == r.ords).all() and (b == r.bits).all(), (name, n)


# ------------------------------------------------------------------------------- the semantic anchor: oracle.fuse
@pytest.mark.parametrize("name,n", ALL)
def test_reference_agrees_with_the_float64_oracle(name, n):
    """Scores within helpers.UNION_TOL of oracle.fuse on the run dicts of the reference's own depth lists, order equal
    outside helpers.UNION_TIE, membership equal."""
    from oracle import oracle

    case, S, D = fc.get(name, n)
    alpha, so = case["alpha"], case["self_ord"]
    r = fr.fuse(S, D, case["depth"], alpha, so)
    nq = len(r.cnt)
    qids = [str(int(so[i])) if so is not None and so[i] >= 0 else f"q{i}" for i in range(nq)]
    assert len(set(qids)) == nq
    runs = []
    for lists in (r.d_lists, r.s_lists):
        runs.append(oracle.get_run_dict(qids, [[float(np.float32(x)) for x in sc] for _, sc in lists],
                                        [[str(int(o)) for o in od] for od, _ in lists], True))
    want = oracle.fuse(runs, [alpha, 1 - alpha])
    worst = 0.0
    for i, qid in enumerate(qids):
        c = int(r.cnt[i])
        got = [str(int(o)) for o in r.ords[i, :c]]
        assert set(got) == set(want[qid]) and len(set(got)) == c, (name, qid)
        ranked = sorted(want[qid].items(), key=lambda kv: (-float(kv[1]), int(kv[0])))
        fs = r.bits[i, :c].view(np.float32)
        for j, (doc, score) in enumerate(ranked):
            worst = max(worst, abs(float(fs[j]) - float(want[qid][got[j]])))
            assert got[j] == doc or abs(float(want[qid][got[j]]) - float(score)) <= helpers.UNION_TIE, (name, qid, j)
    assert worst <= helpers.UNION_TOL, worst


# ------------------------------------------------------------------------------------------- discriminating power
WRONG = {"quotient": fr.Variant(recip=False), "no exact 1": fr.Variant(exact_one=False),
         "separate multiply + add": fr.Variant(fused_add=False), "f32 comparison": fr.Variant(u32_cmp=False),
         "filtered range": fr.Variant(unfiltered=False)}
# members of the unions of ALL whose fused bits change, as counted when the cases were written (91 997 members in all):
#   quotient 18 425, no exact 1 38, separate multiply + add 2 015, f32 comparison 10, filtered range 744
# and 189 of the top-k cuts the GPU tests make (the cases' ks) fall between two members with bit-equal fused scores.
# The floors asserted below are those counts rounded down; the named cases are the ones that a kernel with that one rule
# wrong fails in tests/test_fusion_exact.py (whole unions are compared there: every changed member is a failure).
FLOORS = {"quotient": 18000, "no exact 1": 30, "separate multiply + add": 2000, "f32 comparison": 10, "filtered range": 700}
NAMED = {"quotient": "random_f32", "no exact 1": "mirror_tie", "separate multiply + add": "depth_1024",
         "f32 comparison": "large_sparse", "filtered range": "self_extremes"}
TIE_CUTS_FLOOR = 150


@pytest.fixture(scope="module")
def power():
    changed = {k: {} for k in WRONG}
    members = cuts = 0
    for name, n in ALL:
        case, S, D = fc.get(name, n)
        r = fr.fuse(S, D, case["depth"], case["alpha"], case["self_ord"])
        members += int(r.cnt.sum())
        for k in case["ks"]:
            if k < r.bits.shape[1]:
                inside = k < r.cnt
                cuts += int((r.bits[inside, k - 1] == r.bits[inside, k]).sum())
        for what, v in WRONG.items():
            w = fr.fuse(S, D, case["depth"], case["alpha"], case["self_ord"], v=v)
            changed[what][(name, n)] = int((w.bits != r.bits).sum())
    return changed, members, cuts


@pytest.mark.parametrize("what", list(WRONG))
def test_one_wrong_rule_changes_bits(power, what):
    changed, members, _ = power
    total = sum(changed[what].values())
    print(f"{what}: {total} of {members} members change bits")
    assert total >= FLOORS[what], (what, total)
    for n in (fc.N_SMALL, fc.N_TWO_TILES):     # ... on a named case, at both sizes the GPU tests use
        assert changed[what][(NAMED[what], n)] > 0, (what, NAMED[what], n)


def test_cuts_fall_inside_exact_ties(power):
    _, _, cuts = power
    print(f"{cuts} top-k cuts between members with bit-equal fused scores")
    assert cuts >= TIE_CUTS_FLOOR, cuts


def test_half_weights_cannot_tell_the_fused_add():
    """Why the random cases run at alpha = 0.3: with 0.5 both weights are powers of two, both products are exact, and the
    fused add equals the separate multiply and add on every member."""
    case, S, D = fc.get("random_f32", fc.N_SMALL)
    a = fr.fuse(S, D, case["depth"], 0.5, case["self_ord"])
    b = fr.fuse(S, D, case["depth"], 0.5, case["self_ord"], v=fr.Variant(fused_add=False))
    assert (a.bits == b.bits).all()
