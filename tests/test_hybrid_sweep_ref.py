"""tests/sweep_ref.py against tests/fusion_ref.refuse_union on the CPU: a sweep slice is the union of ONE scoring re-fused
at another alpha. The union arrays come from fuse() at the case's own alpha, the re-fusion runs at every alpha of A9 and
has to give fuse()'s own bits at that alpha: the member sets, src bits, scores and extremes are alpha-independent, which
is what msr_hybrid_sweep relies on. Every assertion is an equality."""
import numpy as np
import pytest

from tests import fusion_cases as fc
from tests import fusion_ref as fr
from tests import sweep_ref as sr

CASES = ["random_f32", "large_sparse", "self_extremes", "short_lists", "full_union"]


def _get(name):
    if name == "full_union":
        return sr.full_union(fc.N_SMALL)
    return fc.get(name, fc.N_SMALL)


@pytest.mark.parametrize("name", CASES)
def test_sweep_is_the_refused_union(name):
    case, S, D = _get(name)
    depth, so = case["depth"], case["self_ord"]
    base = fr.fuse(S, D, depth, case["alpha"], so)
    smax_u = np.asarray(S).max(axis=1)             # the exact maximum of the unfiltered sparse list (0: no hit)
    ords, bits, cnt = sr.sweep(S, D, depth, sr.A9, so, 2 * depth)
    top10 = set()
    for a, alpha in enumerate(sr.A9):
        at = fr.fuse(S, D, depth, alpha, so)
        # alpha-independent: members (as sets), provenance, scores, extremes
        assert (at.cnt == base.cnt).all()
        for i in range(len(at.cnt)):
            c = int(at.cnt[i])
            oa, ob = np.argsort(at.ords[i, :c]), np.argsort(base.ords[i, :c])
            assert (at.ords[i, :c][oa] == base.ords[i, :c][ob]).all()
            assert (at.src[i, :c][oa] == base.src[i, :c][ob]).all()
            assert (at.su[i, :c][oa] == base.su[i, :c][ob]).all()
            assert (at.de[i, :c][oa].view(np.uint32) == base.de[i, :c][ob].view(np.uint32)).all()
        assert (at.rng.view(np.uint32) == base.rng.view(np.uint32)).all()
        r_ords, r_bits = fr.refuse_union(base.ords, base.cnt, base.src, base.su, base.de, base.rng, alpha, smax_u=smax_u)
        assert (r_ords == ords[a]).all() and (r_bits == bits[a]).all() and (cnt[a] == base.cnt).all(), (name, alpha)
        assert (ords[a] == at.ords).all() and (bits[a] == at.bits).all()
        top10.add(ords[a][:, :10].tobytes())
    if name == "random_f32":
        assert len(top10) == len(sr.A9)            # the grid bites: nine different top-10 lists


def test_slices_are_prefixes():
    case, S, D = fc.get("random_f32", fc.N_SMALL)
    full = sr.sweep(S, D, case["depth"], sr.A9, case["self_ord"], 2 * case["depth"])
    for k in (1, 10, 65):
        o, b, c = sr.sweep(S, D, case["depth"], sr.A9, case["self_ord"], k)
        assert o.shape == (len(sr.A9), S.shape[0], k)
        assert (c == np.minimum(full[2], k)).all()
        valid = np.arange(k)[None, None, :] < c[:, :, None]
        assert (o == np.where(valid, full[0][:, :, :k], fr.PAD)).all()
        assert (b == np.where(valid, full[1][:, :, :k], 0)).all()


def test_full_union_fills_the_sort():
    case, S, D = sr.full_union(fc.N_SMALL)
    s2, d2 = fc.scores(case)                       # the planted scores are what the case computes
    assert (s2 == S).all() and (d2.view(np.uint32) == D.view(np.uint32)).all()
    assert case["prec"] == "fp16" and case["depth"] == sr.FULL_DEPTH and S.shape[1] == sr.N_FULL_MIN
    ref = fr.fuse(S, D, case["depth"], 0.3, None)
    assert (ref.cnt == 2 * sr.FULL_DEPTH).all()
    assert ((ref.src == 1).sum(axis=1) == sr.FULL_DEPTH).all() and ((ref.src == 2).sum(axis=1) == sr.FULL_DEPTH).all()
    for i in range(len(ref.cnt)):
        distinct = len(np.unique(ref.bits[i]))
        assert sr.FULL_DEPTH < distinct < 2 * sr.FULL_DEPTH        # distinct fused scores AND ties


def test_large_sparse_sees_the_f32_image_mistake():
    """Deciding t_s = 1 on the f32 image of the sparse maximum instead of the exact u32 score moves bits at some alpha."""
    case, S, D = fc.get("large_sparse", fc.N_SMALL)
    wrong = fr.Variant(u32_cmp=False)
    differs = []
    for alpha in sr.A9:
        good = fr.fuse(S, D, case["depth"], alpha, case["self_ord"])
        bad = fr.fuse(S, D, case["depth"], alpha, case["self_ord"], v=wrong)
        differs.append(bool((good.bits != bad.bits).any() or (good.ords != bad.ords).any()))
    assert any(differs)
    assert not differs[sr.A9.index(1.0)]           # w_s = 0: the sparse term cannot show
