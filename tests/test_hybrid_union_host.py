"""msr_hybrid_search_union, host side: fusion.union_to_runs / union_to_statistic on hand-built union arrays against
fusion.fuse / fusion.fuse_statistic (both pinned to the reference) applied to the lists the arrays describe, the C-ABI
refusal without handles, and the contradictions of `search --fusion_union`, which exit before any GPU work."""
import ctypes

import numpy as np
import pytest

PAD = 0xFFFFFFFF


def _f32(x):
    return np.float32(x)


def _union_arrays():
    """Three queries over ten docs, depth 3 (rows of 6), alpha 0.5, built the way the kernel defines its outputs; the
    fused column is np.float32 of fusion.fuse (pinned to the reference) on the described lists, rows by that value
    descending, ties to the lower ordinal.
    q0: remove_query took the sparse list's best doc (ordinal 2), one doc in both lists, one dense-only doc at the dense
        minimum whose fused score is 0, one sparse-only doc at the sparse minimum (fused 0 as well);
    q1: two docs in both lists, lists of different lengths (the sparse list holds only two docs);
    q2: an empty sparse list (no query term in the vocabulary): dense docs only."""
    from mllm_sparse_retrieval_amd import fusion

    table = np.array([f"d{i:02d}" for i in range(10)], dtype=object)
    qids = ["d02", "q1", "q2"]
    alpha = 0.5
    # per query: dense list [(ord, score)] best first, sparse list [(ord, u32 score)] best first, self ordinal
    lists = [
        ([(5, 0.9), (7, 0.5), (1, 0.25)], [(2, 400), (7, 300), (9, 100)], 2),
        ([(3, 0.75), (0, 0.5), (4, -0.125)], [(0, 220), (3, 90)], -1),
        ([(8, 0.0625), (6, 0.03125), (1, -0.5)], [], -1),
    ]
    w = 6
    ords = np.full((3, w), PAD, np.uint32)
    fused = np.zeros((3, w), np.float32)
    src = np.zeros((3, w), np.uint8)
    su = np.zeros((3, w), np.uint32)
    de = np.zeros((3, w), np.float32)
    rng = np.zeros((3, 4), np.float32)
    n = np.zeros(3, np.int32)
    want_sparse, want_dense = _described_runs(qids, table, lists)
    ref = fusion.fuse([want_dense, want_sparse], [alpha, 1 - alpha])
    for i, (dl, sl, self_ord) in enumerate(lists):
        dmax, dmin = _f32(dl[0][1]), _f32(dl[-1][1])
        smax, smin = (_f32(sl[0][1]), _f32(sl[-1][1])) if sl else (_f32(0), _f32(0))
        rng[i] = [dmax, dmin, smax, smin]
        members = {}
        for o, s in dl:
            members.setdefault(o, [0, 0, _f32(0)])
            members[o][0] |= 1
            members[o][2] = _f32(s)
        for o, s in sl:
            members.setdefault(o, [0, 0, _f32(0)])
            members[o][0] |= 2
            members[o][1] = s
        members.pop(self_ord, None)
        rows = []
        for o, (bits, s_u, d_f) in members.items():
            f = np.float32(ref[qids[i]][table[o]])
            rows.append((-float(f), o, bits, s_u, d_f, f))
        rows.sort()
        n[i] = len(rows)
        for r, (_, o, bits, s_u, d_f, f) in enumerate(rows):
            ords[i, r], fused[i, r], src[i, r], su[i, r], de[i, r] = o, f, bits, s_u, d_f
    return qids, table, lists, alpha, ords, n, fused, src, su, de, rng


def _described_runs(qids, table, lists):
    """get_run_dict of the lists the arrays describe, remove_query on (the first query's id is a doc id)."""
    from mllm_sparse_retrieval_amd.run import get_run_dict

    d_scores = [np.array([s for _, s in dl], np.float32) for dl, _, _ in lists]
    d_docs = [[table[o] for o, _ in dl] for dl, _, _ in lists]
    s_scores = [[float(np.float32(s)) for _, s in sl] for _, sl, _ in lists]
    s_docs = [[table[o] for o, _ in sl] for _, sl, _ in lists]
    return get_run_dict(qids, s_scores, s_docs, True), get_run_dict(qids, d_scores, d_docs, True)


def test_union_to_runs_equals_the_lists_and_their_fusion():
    from mllm_sparse_retrieval_amd import fusion

    qids, table, lists, alpha, ords, n, fused, src, su, de, rng = _union_arrays()
    sparse_run, dense_run, fusion_run = fusion.union_to_runs(qids, table, ords, n, fused, src, su, de, rng)
    want_sparse, want_dense = _described_runs(qids, table, lists)
    for got, want in ((sparse_run, want_sparse), (dense_run, want_dense)):
        assert list(got) == list(want)
        for q in want:
            assert list(got[q]["docs"]) == list(want[q]["docs"]), q            # same docs, best first
            for d in want[q]["docs"]:
                assert type(got[q]["docs"][d]) is type(want[q]["docs"][d]), (q, d)
                assert np.float32(got[q]["docs"][d]) == np.float32(want[q]["docs"][d]), (q, d)
            for key in ("min_score", "max_score"):                             # over the UNFILTERED list
                assert type(got[q][key]) is type(want[q][key]), (q, key)
                assert np.float32(got[q][key]) == np.float32(want[q][key]), (q, key)
    assert "d02" not in sparse_run["d02"]["docs"] and sparse_run["d02"]["max_score"] == 400.0   # the removed best doc
    assert sparse_run["q2"] == {"docs": {}, "min_score": 0, "max_score": 0}
    want_fused = fusion.fuse([want_dense, want_sparse], [alpha, 1 - alpha])
    assert list(fusion_run) == qids
    for q in qids:
        assert set(fusion_run[q]) == set(want_fused[q]), q
        assert all(type(v) is float for v in fusion_run[q].values())
        for d, v in want_fused[q].items():
            assert np.float32(v) == np.float32(fusion_run[q][d]), (q, d)                # equal as f32
        vals = list(fusion_run[q].values())
        assert vals == sorted(vals, reverse=True)
    assert 0.0 in fusion_run["d02"].values()                                   # a member whose fused score is 0
    # fuse() of the runs that union_to_runs built gives the same fused run again: the three are consistent
    again = fusion.fuse([dense_run, sparse_run], [alpha, 1 - alpha])
    for q in qids:
        assert set(again[q]) == set(fusion_run[q])
        assert all(np.float32(again[q][d]) == np.float32(fusion_run[q][d]) for d in again[q])


def test_union_to_runs_refuses_arrays_in_the_wrong_order():
    from mllm_sparse_retrieval_amd import fusion

    qids, table, lists, alpha, ords, n, fused, src, su, de, rng = _union_arrays()
    with pytest.raises(ValueError, match="member count"):   # (fused scores where the member counts belong)
        fusion.union_to_runs(qids, table, ords, fused, n, src, su, de, rng)


def test_union_to_statistic_equals_fuse_statistic():
    from mllm_sparse_retrieval_amd import fusion

    qids, table, lists, alpha, ords, n, fused, src, su, de, rng = _union_arrays()
    got = fusion.union_to_statistic(qids, table, ords, n, fused, src)
    want_sparse, want_dense = _described_runs(qids, table, lists)
    want = fusion.fuse_statistic([want_dense, want_sparse], [alpha, 1 - alpha])
    assert list(got) == qids
    kinds = set()
    for q in qids:
        assert set(got[q]) == set(want[q]), q
        for d, rec in want[q].items():
            assert isinstance(got[q][d], fusion.ResultRecord)
            assert got[q][d].type == rec.type, (q, d)
            assert type(got[q][d].score) is float
            assert np.float32(rec.score) == np.float32(got[q][d].score), (q, d)
            kinds.add(rec.type)
    assert kinds == {"dense", "sparse", "fuse"}


def test_union_refused_without_handles(built, tmp_path):
    import mllm_sparse_retrieval_amd as m
    from mllm_sparse_retrieval_amd import _cabi

    assert _cabi.MSR_UNION_MAX == 2 * _cabi.MSR_KMAX
    assert "msr_hybrid_search_union" in {name for name, _, _ in _cabi.SYMBOLS}
    L = _cabi.lib()
    dp = np.array([0, 1], dtype=np.uint64)
    path = m.build_index_from_csr(str(tmp_path / "i.idx"), dp, np.array([0], np.uint32), np.array([3], np.uint32), 1,
                                  tile_docs=4096)
    qp, qt, qw = _cabi.as_csr([0, 1], [0], [1])
    q = np.zeros((1, 8), np.float32)
    r2o = np.zeros(1, np.uint32)
    ords, sc, n = np.zeros((1, 2), np.uint32), np.zeros((1, 2), np.float32), np.zeros(1, np.int32)
    ms = (ctypes.c_float * 4)()
    with m.SparseIndex(path, device=-1) as ix:
        rc = L.msr_hybrid_search_union(ix._h, None, _cabi.ptr(qp), _cabi.ptr(qt), _cabi.ptr(qw), _cabi.ptr(q), 1, 1, 1, 0.5,
                                       0, _cabi.ptr(r2o), None, _cabi.ptr(ords), _cabi.ptr(sc), _cabi.ptr(n), None, None,
                                       None, None, ms)
        assert rc == -1 and b"msr_hybrid_search_union" in L.msr_last_error()   # MSR_E_INVAL


# ---------------------------------------------------------------------------------------------------------- CLI
def _search(*args):
    from mllm_sparse_retrieval_amd.cli import main

    with pytest.raises(SystemExit) as e:
        main(["search", *args])
    assert e.value.code not in (0, None)
    return str(e.value)


@pytest.fixture()
def no_gpu_work(monkeypatch):
    """Any attempt to open a device-resident index or a dense handle fails the test."""
    from mllm_sparse_retrieval_amd import dense, searcher

    def boom(*a, **k):
        raise AssertionError("GPU work was started")

    monkeypatch.setattr(searcher.LuceneImpactSearcher, "__init__", boom)
    monkeypatch.setattr(dense.DenseIndex, "__init__", boom)


def test_cli_union_contradictions(tmp_path, no_gpu_work):
    both = ("--sparse_index", str(tmp_path), "--passage_reps", str(tmp_path))
    msg = _search(*both, "--fusion_union", "--host_fusion")
    assert "--fusion_union" in msg and "--host_fusion" in msg
    for which in ("--sparse_index", "--passage_reps"):
        msg = _search(which, str(tmp_path), "--fusion_union")
        assert "--fusion_union" in msg and "--passage_reps" in msg and "--sparse_index" in msg
    for depth in ("1025", "0"):
        msg = _search(*both, "--fusion_union", "--depth", depth)
        assert "--fusion_union" in msg and "--depth" in msg and "1024" in msg


def test_cli_union_refuses_an_unsupported_tile_size(built, tmp_path, no_gpu_work):
    import mllm_sparse_retrieval_amd as m

    dp = np.array([0, 1], dtype=np.uint64)
    m.build_index_from_csr(str(tmp_path / "index"), dp, np.array([0], np.uint32), np.array([3], np.uint32), 1,
                           tile_docs=12288)
    msg = _search("--sparse_index", str(tmp_path / "index"), "--passage_reps", str(tmp_path), "--fusion_union")
    assert "12288" in msg and "--host_fusion" in msg


def test_cli_help_documents_fusion_union(capsys):
    from mllm_sparse_retrieval_amd.cli import main

    with pytest.raises(SystemExit):
        main(["search", "--help"])
    out = " ".join(capsys.readouterr().out.split())
    assert "--fusion_union" in out and "msr_hybrid_search_union" in out
    assert "ignored under --fusion_union" in out
