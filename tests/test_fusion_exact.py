"""The hybrid fusion on the GPU against tests/fusion_ref.py, bit for bit: ordinals, fused score bits, counts and padding of
msr_hybrid_search, msr_hybrid_search_f32 and msr_hybrid_search_union (and the union's side arrays and ranges) on every
back end, told apart by the ms layout as tests/test_hybrid_f32.py does:

    fused4096 / fused8192   one tile, k <= 64: hybrid_tiles (k > 64 and the union take the candidate kernels on one tile)
    multi                   4096-doc tiles, the default quota: hybrid_tiles<MODE 1> + hybrid_fuse_query
    round2                  the same with MSR_HYBRID_QUOTA = 1: every query goes to the second round
    list12288               a 12288-doc tile: the list path (score_tiles, select_tiles, fuse_tiles, merges)
    list_child              MSR_NO_FUSED_HYBRID in a fresh child process: the list path on 4096-doc tiles

Inputs: tests/fusion_cases.py (their CPU side: tests/test_fusion_ref.py). Dense scores are exact on the CPU: the fmaf chain
on f32 handles, exact accumulation of 1/8-multiples on fp16 handles (such a case runs on both handles). The dense tie rule
is the documented one per path: lower ordinal on the candidate paths, lower row on the list path. Every assertion is an
equality."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from tests import fusion_cases as fc
from tests import fusion_ref as fr
from tests import rank_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (tile_docs, docs, forced quota); a case with a size of its own (depth_ge_n) keeps it
BACKENDS = {"fused4096": (4096, fc.N_SMALL, None), "fused8192": (8192, fc.N_TWO_TILES, None),
            "multi": (4096, fc.N_TWO_TILES, None), "round2": (4096, fc.N_TWO_TILES, 1),
            "list12288": (12288, fc.N_TWO_TILES, None)}
CHILD_CASES = [(name, fc.N_TWO_TILES) for name in list(fc.EDGES) + list(fc.RANDOM)]
K_ALL = 1024    # the list path has no union call: its whole union is read through the largest k


@pytest.fixture(scope="module")
def m(built):
    import mllm_sparse_retrieval_amd as m

    return m


def _backend(ms):
    if ms["dense_select"] > 0:
        return "list"
    return "multi" if ms["fusion"] > 0 else "fused"


def _precs(case):
    return ("f32", "fp16") if case["prec"] == "fp16" else ("f32",)


def _ks(case, list_path):
    return tuple(sorted(set(case["ks"]) | ({K_ALL} if list_path else set())))


def gpu_calls(m, workdir, case, tile, list_path):
    """Every entry point on one case -> {(prec, k): (ords, score bits, counts, back end), (prec, "union"): (...)}."""
    from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_search, hybrid_search_f32, hybrid_search_union

    n = len(case["r2o"])
    ids = ["%07d" % o for o in case["r2o"]]                    # doc ids = zero-padded ordinals: ordinal != row
    path = m.build_index_from_csr(os.path.join(str(workdir), f"{case['name']}_{n}_{tile}.idx"),
                                  *rank_ref.docs_to_csr(case["Dm"]), case["Dm"].shape[1], doc_ids=ids, tile_docs=tile)
    qp, qt, qw = rank_ref.csr(case["queries"])
    depth, alpha, r2o, so = case["depth"], case["alpha"], case["r2o"], case["self_ord"]
    out = {}
    with m.SparseIndex(path, device=0) as ix:
        assert ix.docid_table().tolist() == rank_ref.doc_ids(n)
        for prec in _precs(case):
            dix = DenseIndex(case["p"], precision=prec)
            try:
                topk = hybrid_search_f32 if prec == "f32" else hybrid_search
                for k in _ks(case, list_path):
                    o, f, c, ms = topk(ix, dix, qp, qt, qw, case["q"], depth, k, alpha, r2o, so)
                    out[(prec, k)] = (o, f.view(np.uint32), c, _backend(ms))
                if not list_path:
                    u = hybrid_search_union(ix, dix, qp, qt, qw, case["q"], depth, alpha, r2o, so)
                    out[(prec, "union")] = (u[0], u[1].view(np.uint32), u[2], u[3], u[4], u[5].view(np.uint32),
                                            u[6].view(np.uint32), _backend(u[7]))
            finally:
                dix.close()
    os.remove(path)
    return out


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, "first differences at", bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def check(case, S, D, out, tile, list_path):
    """Everything the calls returned against the reference; the dense tie key follows the path."""
    ref = fr.fuse(S, D, case["depth"], case["alpha"], case["self_ord"], row2ord=case["r2o"] if list_path else None)
    n = S.shape[1]
    assert set(p for p, _ in out) == set(_precs(case))
    for (prec, k), res in out.items():
        tag = (case["name"], n, tile, prec, k)
        if k == "union":
            ords, bits, cnt, src, su, de, rng, backend = res
            assert backend == "multi", tag
            _same(cnt, ref.cnt, tag + ("counts",))
            _same(ords, ref.ords, tag + ("ordinals",))                    # padding included: 0xFFFFFFFF
            _same(bits, ref.bits, tag + ("fused score bits",))            # padding included: +0
            _same(src, ref.src, tag + ("src",))
            _same(su, ref.su, tag + ("sparse u32",))
            _same(de, ref.de.view(np.uint32), tag + ("dense bits",))
            _same(rng, ref.rng.view(np.uint32), tag + ("range bits",))
        else:
            ords, bits, cnt, backend = res
            want = "list" if list_path else ("fused" if n <= tile and k <= 64 else "multi")
            assert backend == want, tag + (backend, want)
            w_ords, w_bits, w_cnt = fr.topk(ref, k)
            _same(cnt, w_cnt, tag + ("counts",))
            _same(ords, w_ords, tag + ("ordinals",))
            _same(bits, w_bits, tag + ("fused score bits",))


def _run(m, tmp_path, monkeypatch, name, backend):
    tile, n, quota = BACKENDS[backend]
    if quota:
        monkeypatch.setenv("MSR_HYBRID_QUOTA", str(quota))
    else:
        monkeypatch.delenv("MSR_HYBRID_QUOTA", raising=False)
    case, S, D = fc.get(name, n)
    list_path = tile == 12288
    check(case, S, D, gpu_calls(m, tmp_path, case, tile, list_path), tile, list_path)


# -------------------------------------------------------------------------------------- named edges, every back end
@pytest.mark.parametrize("backend", list(BACKENDS))
@pytest.mark.parametrize("name", list(fc.EDGES))
def test_edge(m, tmp_path, monkeypatch, name, backend):
    """One named edge (tests/fusion_cases.py says what each is) on one in-process back end."""
    _run(m, tmp_path, monkeypatch, name, backend)


# ------------------------------------------------------------------------------------------------ random corpora
@pytest.mark.parametrize("backend", list(BACKENDS))
@pytest.mark.parametrize("name", list(fc.RANDOM))
def test_random(m, tmp_path, monkeypatch, name, backend):
    """24 queries with remove_query, depth 300, alpha 0.3 (inexact products: the fused adds matter), k = 1, 64, 65, 1024
    and the union's 600; normal f32 rows on the fmaf chain and 1/8-multiples on both handles."""
    _run(m, tmp_path, monkeypatch, name, backend)


@pytest.mark.parametrize("quota", [None, 3])
@pytest.mark.parametrize("name", list(fc.RANDOM))
def test_random_five_tiles(m, tmp_path, monkeypatch, name, quota):
    """4 tiles of 4096 docs and a last tile of ONE doc, with the default quota and with every query in the second round."""
    if quota:
        monkeypatch.setenv("MSR_HYBRID_QUOTA", str(quota))
    else:
        monkeypatch.delenv("MSR_HYBRID_QUOTA", raising=False)
    case, S, D = fc.get(name, fc.N_FIVE_TILES)
    check(case, S, D, gpu_calls(m, tmp_path, case, 4096, False), 4096, False)


# ------------------------------------------------------------------------- the list path forced in a child process
def child_main(out_path, workdir):
    """Runs in the child (MSR_NO_FUSED_HYBRID is read once per process): every child case through the top-k calls."""
    import mllm_sparse_retrieval_amd as m

    res = {}
    for name, n in CHILD_CASES:
        case, _, _ = fc.get(name, n)
        res[name] = gpu_calls(m, workdir, case, 4096, True)
    with open(out_path, "wb") as f:
        pickle.dump(res, f)


@pytest.fixture(scope="module")
def child_out(m, tmp_path_factory):
    work = tmp_path_factory.mktemp("list_child")
    out_path = str(work / "out.pkl")
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_fusion_exact import child_main; "
            f"child_main({out_path!r}, {str(work)!r})")
    env = dict(os.environ, MSR_NO_FUSED_HYBRID="1")
    env.pop("MSR_HYBRID_QUOTA", None)
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300, env=env)
    with open(out_path, "rb") as f:
        return pickle.load(f)


@pytest.mark.parametrize("name", [name for name, _ in CHILD_CASES])
def test_list_child(child_out, name):
    """MSR_NO_FUSED_HYBRID sends an index the candidate path would take (4096-doc tiles) down the list path: the same
    bits, with the list path's dense tie rule (lower row)."""
    case, S, D = fc.get(name, dict(CHILD_CASES)[name])
    check(case, S, D, child_out[name], 4096, True)


# ------------------------------------------------------------------------------------------------------- fuzz
def test_fuzz(m, tmp_path, monkeypatch):
    """Seeded draws of planted scores (density, score range, dense value range, depth 1-1024, alpha in and outside
    [0, 1], self_ord, k) over every in-process back end and the sizes at their edges: a full tile, a last tile of one
    doc, three tiles. MSR_FUZZ_SEED / MSR_FUZZ_CASES as in the other fuzz tests."""
    rng = np.random.default_rng(int(os.environ.get("MSR_FUZZ_SEED", "20261018")))
    for i in range(int(os.environ.get("MSR_FUZZ_CASES", "16"))):
        tile = int(rng.choice([4096, 8192, 12288]))
        n = int(rng.choice([fc.N_SMALL, 4097] if tile == 12288 else [fc.N_SMALL, tile, tile + 1, 2 * tile + 1]))
        if i % 3 == 2:
            monkeypatch.setenv("MSR_HYBRID_QUOTA", str(int(rng.integers(1, 41))))
        else:
            monkeypatch.delenv("MSR_HYBRID_QUOTA", raising=False)
        case = fc.fuzz_case(rng, n)
        case["name"] = f"fuzz{i}"
        S, D = fc.scores(case)
        check(case, S, D, gpu_calls(m, tmp_path, case, tile, tile == 12288), tile, tile == 12288)
    monkeypatch.delenv("MSR_HYBRID_QUOTA", raising=False)
