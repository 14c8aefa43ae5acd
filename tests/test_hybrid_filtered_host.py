"""msr_hybrid_deep_filtered, host side: the symbol in the header, the library and the binding; the refusal of a call
without a dense handle before any range or device check; dense.hybrid_deep_filtered's refusals before the library is
touched; the contradictions, the depth range and the warning of `search --fusion_filtered`, which come before any GPU work;
the refusals that stay and now name the flag; --help."""
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
    assert "int msr_hybrid_deep_filtered(msr_index* ix, msr_dense* dx," in header
    assert "const uint32_t* set_bits, int n_sets, const int32_t* q_set," in header and "float ms[7]" in header
    bound = {name: (res, args) for name, res, args in _cabi.SYMBOLS}
    assert len(bound["msr_hybrid_deep_filtered"][1]) == len(bound["msr_hybrid_deep"][1]) + 3 == 31
    # the three set arguments sit after self_ord (argument 15 of both calls)
    assert bound["msr_hybrid_deep_filtered"][1][15:18] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    assert bound["msr_hybrid_deep_filtered"][1][:15] + bound["msr_hybrid_deep_filtered"][1][18:] == bound["msr_hybrid_deep"][1]
    assert hasattr(ctypes.CDLL(_cabi.LIB_PATH), "msr_hybrid_deep_filtered")
    assert _cabi.lib().msr_hybrid_deep_filtered.argtypes == bound["msr_hybrid_deep_filtered"][1]


def test_filtered_refused_without_handles(built, tmp_path):
    """A device = -1 index handle: MSR_E_INVAL (no dense handle; malformed sets) comes before MSR_E_RANGE and
    MSR_E_NODEVICE, and msr_last_error names the call."""
    import mllm_sparse_retrieval_amd as m
    from mllm_sparse_retrieval_amd import _cabi

    L = _cabi.lib()
    path = m.build_index_from_csr(str(tmp_path / "i.idx"), np.array([0, 1], dtype=np.uint64), np.array([0], np.uint32),
                                  np.array([3], np.uint32), 1, tile_docs=4096)
    qp, qt, qw = _cabi.as_csr([0, 1], [0], [1])
    q, r2o, al = np.zeros((1, 8), np.float32), np.zeros(1, np.uint32), np.array([0.5], np.float32)
    ords, sc, n = np.zeros((1, 1, 2), np.uint32), np.zeros((1, 1, 2), np.float32), np.zeros((1, 1), np.int32)
    mem, bits, qs = np.zeros(1, np.uint32), np.ones((2, 1), np.uint32), np.zeros(1, np.int32)
    ms = (ctypes.c_float * 7)()
    p = _cabi.ptr
    with m.SparseIndex(path, device=-1) as ix:
        for depth, k, n_alphas, n_sets in ((1, 2, 1, 1), (0, 0, 0, 1 << 20), (1 << 20, 1, 65, -1)):
            rc = L.msr_hybrid_deep_filtered(ix._h, None, p(qp), p(qt), p(qw), p(q), 1, 1, depth, k, p(al), n_alphas, 0, p(r2o),
                                            None, p(bits), n_sets, p(qs), p(ords), p(sc), p(n), p(mem), None, None, None, None,
                                            None, None, None, None, ms)
            assert rc == -1 and b"msr_hybrid_deep_filtered" in L.msr_last_error()     # MSR_E_INVAL: no dense handle
        rc = L.msr_hybrid_deep_filtered(None, None, p(qp), p(qt), p(qw), p(q), 1, 1, 1, 2, p(al), 1, 0, p(r2o), None, None, 0,
                                        None, p(ords), p(sc), p(n), p(mem), None, None, None, None, None, None, None, None,
                                        None)
        assert rc == -1 and b"msr_hybrid_deep_filtered" in L.msr_last_error()


# ------------------------------------------------------------------------------- dense.hybrid_deep_filtered's own checks
@pytest.fixture()
def no_library(monkeypatch):
    """Any call into libmsr fails the test."""
    from mllm_sparse_retrieval_amd import dense

    def boom(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(dense, "lib", boom)


@pytest.mark.parametrize("prec", ["fp16", "f32"])
def test_hybrid_deep_filtered_refuses_before_the_library(no_library, prec):
    from mllm_sparse_retrieval_amd.dense import hybrid_deep_filtered
    from mllm_sparse_retrieval_amd.filters import pack_doc_sets

    ix = SimpleNamespace(_h=None, n_docs=5)
    dix = SimpleNamespace(_h=None, precision=prec, dim=8, n=5)
    qp, qt, qw = [0, 1, 2], [0, 1], [1, 1]
    q, r2o = np.zeros((2, 8), np.float32), np.arange(5, dtype=np.uint32)
    two = np.array([[1, 0, 1, 0, 1], [0, 1, 0, 1, 0]], dtype=bool)

    def call(q_ptr=qp, q_term=qt, q_w=qw, q_reps=q, depth=4, k=8, alphas=(0.0, 0.5), row2ord=r2o, sets=two, q_set=(0, -1),
             self_ord=None):
        return hybrid_deep_filtered(ix, dix, q_ptr, q_term, q_w, q_reps, depth, k, alphas, row2ord, sets, q_set, self_ord)

    for bad, match in ((dict(sets=np.ones((2, 6), bool)), "bool doc sets need shape"),
                       (dict(sets=np.ones((2, 5), np.int64)), "bool .* or packed uint32"),
                       (dict(sets=np.ones((2, 2), np.uint32)), "packed doc sets need shape"),
                       (dict(q_set=None), "q_set is required"),
                       (dict(q_set=(0, 1, 0)), "one entry per query"),
                       (dict(q_reps=np.zeros((2, 16), np.float32)), "dimension mismatch"),
                       (dict(q_reps=np.zeros((3, 8), np.float32)), "query counts differ"),
                       (dict(q_ptr=[0, 1, 3]), "malformed CSR"),
                       (dict(row2ord=np.arange(4, dtype=np.uint32)), "row2ord"),
                       (dict(self_ord=np.zeros(3, np.int32)), "self_ord"),
                       (dict(k=0), "k must be"), (dict(k=9), "k must be"), (dict(depth=16384, k=16385), "k must be"),
                       (dict(depth=0), "depth must be"), (dict(depth=16385, k=1), "depth must be"),
                       (dict(alphas=[]), "alphas"), (dict(alphas=[0.1] * 65), "alphas"),
                       (dict(alphas=[0.1, float("nan")]), "finite")):
        with pytest.raises(ValueError, match=match):
            call(**bad)
    # well-formed calls reach the library: bool and packed sets, one set without q_set, no set at all
    for good in (dict(), dict(sets=pack_doc_sets(two)), dict(sets=two[0], q_set=None), dict(sets=two[:0], q_set=None),
                 dict(depth=16384, k=16384)):
        with pytest.raises(AssertionError, match="the library was called"):
            call(**good)


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


def test_cli_fusion_filtered_contradictions(tmp_path, monkeypatch, no_gpu_work):
    both = ("--sparse_index", str(tmp_path), "--passage_reps", str(tmp_path))
    sets = ("--doc_sets", str(tmp_path / "d"), "--query_sets", str(tmp_path / "q"))
    for which in ("--sparse_index", "--passage_reps"):
        msg = _search(which, str(tmp_path), "--fusion_filtered", *sets)
        assert "--fusion_filtered" in msg and "--passage_reps" in msg and "--sparse_index" in msg
    for part in ((), sets[:2], sets[2:]):
        msg = _search(*both, "--fusion_filtered", *part)
        assert "--fusion_filtered needs both --doc_sets" in msg and "--query_sets" in msg
    for flag, extra in (("--host_fusion", ()), ("--fusion_union", ()), ("--fusion_deep", ()), ("--deep", ()), ("--ranks", ()),
                        ("--explain", ("3",))):
        for grid in ((), ("--alphas", "0,1")):
            msg = _search(*both, "--fusion_filtered", *sets, *grid, flag, *extra)
            assert "--fusion_filtered does not combine with " + flag in msg, (flag, msg)
    for depth in ("0", "16385", "-3"):
        msg = _search(*both, "--fusion_filtered", *sets, "--depth", depth)
        assert "--fusion_filtered" in msg and "--depth" in msg and "16384" in msg, msg
    for text, why in (("", "empty"), ("0,x,1", "not a number"), ("0,nan", "not finite"),
                      (",".join(str(i / 100) for i in range(65)), "at most MSR_SWEEP_MAX_ALPHAS = 64")):
        msg = _search(*both, "--fusion_filtered", *sets, "--alphas=" + text)
        assert "--alphas" in msg and why in msg, (text, msg)
    msg = _search(*both, "--fusion_filtered", *sets, "--sweep_runs")
    assert "--sweep_runs" in msg and "--alphas" in msg
    msg = _search(*both, "--fusion_filtered", *sets, "--hybrid_f32", "--use_gpu")
    assert "--hybrid_f32" in msg and "--use_gpu" in msg
    monkeypatch.setenv("WORLD_SIZE", "2")
    msg = _search(*both, "--fusion_filtered", *sets)
    assert "--fusion_filtered" in msg and "WORLD_SIZE" in msg


def test_cli_existing_refusals_stay_and_name_the_flag(tmp_path, no_gpu_work):
    both = ("--sparse_index", str(tmp_path), "--passage_reps", str(tmp_path))
    sets = ("--doc_sets", str(tmp_path / "d"), "--query_sets", str(tmp_path / "q"))
    msg = _search(*both, "--fusion_deep", *sets)
    assert "--fusion_deep does not combine with --doc_sets / --query_sets" in msg and "--fusion_filtered" in msg
    msg = _search(*both, *sets)
    assert "filtered hybrid" in msg and "--host_fusion" in msg and "--fusion_filtered" in msg
    msg = _search(*both, "--alphas", "0,1", *sets)
    assert "--alphas does not combine with --doc_sets / --query_sets" in msg and "--fusion_filtered" in msg
    msg = _search(*both, "--host_fusion", "--depth", "2000", *sets)
    assert "filtered search needs --depth in [1, MSR_KMAX = 1024]" in msg


@pytest.mark.parametrize("depth,warns", [("8192", False), ("8193", True), ("16384", True), ("2000", False)])
def test_cli_fusion_filtered_warning_and_then_the_gpu(tmp_path, capsys, monkeypatch, no_gpu_work, depth, warns):
    """A well-formed command passes every check and only then reaches the searcher; 2 x depth > 16384 warns first."""
    import glob

    import mllm_sparse_retrieval_amd.run as run
    from mllm_sparse_retrieval_amd import cli

    monkeypatch.setattr(glob, "glob", lambda pat: ["corpus.pkl"])
    monkeypatch.setattr(run, "pickle_load", lambda path: (np.zeros((1, 8), np.float32), ["0"]))
    with pytest.raises(AssertionError, match="GPU work was started"):
        cli.main(["search", "--sparse_index", str(tmp_path), "--passage_reps", str(tmp_path), "--fusion_filtered", "--doc_sets",
                  str(tmp_path / "d"), "--query_sets", str(tmp_path / "q"), "--depth", depth, "--alphas", "0,0.5",
                  "--hybrid_f32", "--remove_query"])
    err = capsys.readouterr().err
    assert (("WARNING" in err and "--fusion_filtered" in err and "16384" in err and str(2 * int(depth)) in err) if warns
            else "WARNING" not in err), err


def test_cli_help_documents_fusion_filtered(capsys):
    from mllm_sparse_retrieval_amd.cli import main

    with pytest.raises(SystemExit):
        main(["search", "--help"])
    out = " ".join(capsys.readouterr().out.split())
    assert "--fusion_filtered" in out and "msr_hybrid_deep_filtered" in out and "16384" in out
    assert "--doc_sets FILE --query_sets FILE" in out
