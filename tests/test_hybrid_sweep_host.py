"""msr_hybrid_sweep, host side: the symbol in the header, the library and the binding; dense.hybrid_sweep's refusals before
the library is touched; recall.sweep_recall against RecallMetrics on seeded lists; the contradictions of `search --alphas`,
which exit with their message before any GPU work; --help."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------ the symbol
def test_symbol_declared_exported_and_bound(built):
    from mllm_sparse_retrieval_amd import _cabi

    with open(os.path.join(ROOT, "include", "msr.h")) as f:
        header = f.read()
    assert "int msr_hybrid_sweep(msr_index* ix, msr_dense* dx," in header
    assert "#define MSR_SWEEP_MAX_ALPHAS 64" in header and _cabi.MSR_SWEEP_MAX_ALPHAS == 64
    bound = {name: (res, args) for name, res, args in _cabi.SYMBOLS}
    assert "msr_hybrid_sweep" in bound and len(bound["msr_hybrid_sweep"][1]) == 19
    assert hasattr(ctypes.CDLL(_cabi.LIB_PATH), "msr_hybrid_sweep")
    assert _cabi.lib().msr_hybrid_sweep.argtypes == bound["msr_hybrid_sweep"][1]


def test_sweep_refused_without_handles(built, tmp_path):
    import mllm_sparse_retrieval_amd as m
    from mllm_sparse_retrieval_amd import _cabi

    L = _cabi.lib()
    path = m.build_index_from_csr(str(tmp_path / "i.idx"), np.array([0, 1], dtype=np.uint64), np.array([0], np.uint32),
                                  np.array([3], np.uint32), 1, tile_docs=4096)
    qp, qt, qw = _cabi.as_csr([0, 1], [0], [1])
    q, r2o, al = np.zeros((1, 8), np.float32), np.zeros(1, np.uint32), np.array([0.5], np.float32)
    ords, sc, n = np.zeros((1, 1, 2), np.uint32), np.zeros((1, 1, 2), np.float32), np.zeros((1, 1), np.int32)
    ms = (ctypes.c_float * 6)()
    with m.SparseIndex(path, device=-1) as ix:
        rc = L.msr_hybrid_sweep(ix._h, None, _cabi.ptr(qp), _cabi.ptr(qt), _cabi.ptr(qw), _cabi.ptr(q), 1, 1, 1, 2,
                                _cabi.ptr(al), 1, 0, _cabi.ptr(r2o), None, _cabi.ptr(ords), _cabi.ptr(sc), _cabi.ptr(n), ms)
        assert rc == -1 and b"msr_hybrid_sweep" in L.msr_last_error()   # MSR_E_INVAL: no dense handle


# -------------------------------------------------------------------------------------- dense.hybrid_sweep's own checks
@pytest.fixture()
def no_library(monkeypatch):
    """Any call into libmsr fails the test."""
    from mllm_sparse_retrieval_amd import dense

    def boom(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(dense, "lib", boom)


@pytest.mark.parametrize("prec", ["fp16", "f32"])
def test_hybrid_sweep_refuses_before_the_library(no_library, prec):
    from mllm_sparse_retrieval_amd.dense import hybrid_sweep

    ix = SimpleNamespace(_h=None)
    dix = SimpleNamespace(_h=None, precision=prec, dim=8, n=5)
    qp, qt, qw = [0, 1, 2], [0, 1], [1, 1]
    q, r2o = np.zeros((2, 8), np.float32), np.arange(5, dtype=np.uint32)

    def call(q_ptr=qp, q_term=qt, q_w=qw, q_reps=q, depth=4, k=8, alphas=(0.0, 0.5), row2ord=r2o, self_ord=None):
        return hybrid_sweep(ix, dix, q_ptr, q_term, q_w, q_reps, depth, k, alphas, row2ord, self_ord)

    for bad, match in ((dict(q_reps=np.zeros((2, 16), np.float32)), "dimension mismatch"),
                       (dict(q_reps=np.zeros((3, 8), np.float32)), "query counts differ"),
                       (dict(q_reps=np.zeros(8, np.float32)), "matrix"),
                       (dict(q_ptr=[0, 1, 3]), "malformed CSR"),
                       (dict(row2ord=np.arange(4, dtype=np.uint32)), "row2ord"),
                       (dict(self_ord=np.zeros(3, np.int32)), "self_ord"),
                       (dict(k=0), "k must be"), (dict(k=9), "k must be"),
                       (dict(depth=0), "depth must be"), (dict(depth=1025, k=1), "depth must be"),
                       (dict(alphas=[]), "alphas"), (dict(alphas=[0.1] * 65), "alphas"),
                       (dict(alphas=[[0.1, 0.2]]), "alphas"),
                       (dict(alphas=[0.1, float("nan")]), "finite"), (dict(alphas=[float("inf")]), "finite")):
        with pytest.raises(ValueError, match=match):
            call(**bad)
    with pytest.raises(AssertionError, match="the library was called"):   # a well-formed call reaches the library
        call()


# -------------------------------------------------------------------------------------------------- sweep_recall
class _Qrels:
    def __init__(self, targets):
        self.targets = targets

    def get_target(self, qid, query_type):
        return self.targets[qid]


def test_sweep_recall_equals_recall_metrics():
    from mllm_sparse_retrieval_amd.recall import RECALL_KS, RecallMetrics, sweep_recall

    rng = np.random.default_rng(5)
    n_a, nq, k, n_docs = 3, 40, 250, 400
    docid = np.array([str(3 * o + 1) for o in range(n_docs)], dtype=object)      # doc id != ordinal
    ords = np.stack([np.stack([rng.permutation(n_docs)[:k] for _ in range(nq)]) for _ in range(n_a)]).astype(np.uint32)
    n = rng.integers(0, k + 1, (n_a, nq)).astype(np.int32)
    n[:, 0] = 0                                                                    # a query without docs
    n[:, 1] = k
    qids = [f"q{i}" for i in range(nq)]
    t_ord = [rng.choice(n_docs, int(rng.integers(1, 6)), replace=False).tolist() for _ in range(nq)]
    t_ord[2] = [int(x) for x in np.setdiff1d(np.arange(n_docs), ords[:, 2].ravel())[:2]]   # no hit at any alpha
    n[0, 3], t_ord[3] = 7, [int(ords[0, 3, 7])]                                   # the target sits just past n
    t_ord[4] = [int(ords[1, 4, 0]), int(ords[2, 4, 150]), int(ords[0, 4, 4])]     # several targets
    n[:, 4] = k
    t_ord[5] = [int(ords[0, 5, 0])]                                               # a single, non-list target
    n[0, 5] = 1
    targets = {q: ([str(docid[o]) for o in t] if i != 5 else str(docid[t_ord[5][0]])) for i, (q, t) in enumerate(zip(qids, t_ord))}
    ords_pad = ords.copy()
    for a in range(n_a):
        for i in range(nq):
            ords_pad[a, i, n[a, i]:] = 0xFFFFFFFF
    got = sweep_recall(ords_pad, n, t_ord)
    assert got.shape == (n_a, len(RECALL_KS)) and got.dtype == np.int64
    args = SimpleNamespace(query_type="text")
    for a in range(n_a):
        run = {q: {docid[o]: float(k - c) for c, o in enumerate(ords[a, i, :n[a, i]])} for i, q in enumerate(qids)}
        m = RecallMetrics(_Qrels(targets), {}, {}, run, [], qids, args)
        m.sort_and_count()
        m.all_gather_object()
        want = m.recalls()["fusion"]
        assert [c / nq for c in got[a].tolist()] == [want[kk] for kk in RECALL_KS], a
    assert got[0, RECALL_KS.index(200)] < nq                                       # some query misses: the test bites
    assert (np.diff(got, axis=1) >= 0).all()
    with pytest.raises(ValueError, match="sweep_recall"):
        sweep_recall(ords_pad, n[:, :-1], t_ord)


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


def test_cli_sweep_contradictions(tmp_path, monkeypatch, no_gpu_work):
    both = ("--sparse_index", str(tmp_path), "--passage_reps", str(tmp_path))
    grid = ("--alphas", "0,0.5,1")
    for which in ("--sparse_index", "--passage_reps"):
        msg = _search(which, str(tmp_path), *grid)
        assert "--alphas" in msg and "--passage_reps" in msg and "--sparse_index" in msg
    for flag, extra in (("--host_fusion", ()), ("--fusion_union", ()), ("--deep", ()), ("--ranks", ()), ("--explain", ("3",))):
        msg = _search(*both, *grid, flag, *extra)
        assert "--alphas does not combine with " + flag in msg, (flag, msg)
    msg = _search(*both, *grid, "--doc_sets", str(tmp_path / "d"), "--query_sets", str(tmp_path / "q"))
    assert "--alphas does not combine with --doc_sets / --query_sets" in msg
    for depth in ("1025", "0"):
        msg = _search(*both, *grid, "--depth", depth)
        assert "--alphas" in msg and "--depth" in msg and "1024" in msg
    for text, why in (("", "empty"), (",", "empty"), ("0,x,1", "not a number"), ("0,nan", "not finite"),
                      ("1e39", "not finite"), (",".join(str(i / 100) for i in range(65)), "at most MSR_SWEEP_MAX_ALPHAS = 64"),
                      (",".join(str(1 + i / 100) for i in range(64)), "at most MSR_SWEEP_MAX_ALPHAS = 64")):   # 64 + --alpha
        msg = _search(*both, "--alphas=" + text)
        assert "--alphas" in msg and why in msg, (text, msg)
    msg = _search(*both, "--sweep_runs")
    assert "--sweep_runs" in msg and "--alphas" in msg
    monkeypatch.setenv("WORLD_SIZE", "2")
    msg = _search(*both, *grid)
    assert "--alphas" in msg and "WORLD_SIZE" in msg


def test_parse_alphas_adds_alpha_once():
    from mllm_sparse_retrieval_amd.cli import parse_alphas

    assert parse_alphas("0,0.3,1", 0.5) == [0.0, 0.3, 1.0, 0.5]
    assert parse_alphas("0, 0.5 ,1", 0.5) == [0.0, 0.5, 1.0]
    assert parse_alphas("0.3,0.3", 0.3) == [0.3, 0.3]                 # duplicates stay
    assert parse_alphas("-0.25,1.5", 1.5) == [-0.25, 1.5]
    assert len(parse_alphas(",".join(str(i / 100) for i in range(64)), 0.5)) == 64


def test_cli_sweep_refuses_an_unsupported_tile_size(built, tmp_path, no_gpu_work):
    import mllm_sparse_retrieval_amd as m

    m.build_index_from_csr(str(tmp_path / "index"), np.array([0, 1], dtype=np.uint64), np.array([0], np.uint32),
                           np.array([3], np.uint32), 1, tile_docs=12288)
    msg = _search("--sparse_index", str(tmp_path / "index"), "--passage_reps", str(tmp_path), "--alphas", "0,1")
    assert "--alphas" in msg and "12288" in msg and "4096" in msg


def test_cli_help_documents_the_sweep(capsys):
    from mllm_sparse_retrieval_amd.cli import main

    with pytest.raises(SystemExit):
        main(["search", "--help"])
    out = " ".join(capsys.readouterr().out.split())
    assert "--alphas" in out and "msr_hybrid_sweep" in out and "--sweep_runs" in out
    assert "fusion.sweep.tsv" in out and "fusion.alpha_{a}.trec" in out
