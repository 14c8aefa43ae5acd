"""The numpy reference of msr_explain_docs (tests/explain_ref.py) satisfies the call's identity against the reference of
msr_rank_docs (tests/rank_ref.py): sum_j max(omega_j, 0) * w(tau_j, t) == S[q, t]. No library call."""
import numpy as np
import pytest

from tests import explain_ref as er
from tests import rank_ref as rr


@pytest.mark.parametrize("drop", [True, False])
def test_reference_satisfies_the_identity(drop):
    D = rr.random_corpus(500, 60, 12, seed=5)
    rows = rr.random_queries(20, 8, 60, seed=6) + [[], [(0, 3)], [(-1, 2), (7, 0), (9, -4)]]
    tg = rr.random_targets(len(rows), 500, seed=7)
    tg[20] = [3, 4]                                        # a query without entries that lists docs: zero slots
    assert any(len(x) == 0 for x in tg) and any(len(set(x)) < len(x) for x in tg)
    q, t = rr.csr(rows), rr.targets_csr(tg)
    xp, w = er.explain(*q, *t, D, drop)
    S = rr.scores(*q, D, drop)
    _, want = rr.ranks(S, *t)
    assert len(xp) == len(t[1]) + 1 and xp[-1] == len(w) == sum(len(r) * len(g) for r, g in zip(rows, tg))
    assert (er.row_scores(q[0], q[2], t[0], xp, w) == want).all() and want.max() > 0
    # the planted dirty entries (OOV, zero and negative weight) never carry a weight; the df == N term only when kept
    ok = er.counts(*q, D, drop)
    for i in range(len(rows)):
        for e in range(t[0][i], t[0][i + 1]):
            assert (w[xp[e]:xp[e + 1]][~ok[q[0][i]:q[0][i + 1]]] == 0).all()
    has0 = [any(a == 0 and b > 0 for a, b in r) for r in rows]
    assert any(has0) and ok[np.asarray(q[1]) == 0].any() == (not drop)
