"""msr_hybrid_sweep (dense.hybrid_sweep, search --alphas) on the GPU, bit for bit: against tests/sweep_ref.py (= fusion_ref
per alpha), against msr_hybrid_search[_f32] and msr_hybrid_search_union at every alpha, independence of the alpha list,
alpha groups beyond one staging buffer, the steady state of the scratch, every refusal with its code, and the CLI against
plain runs. Inputs: tests/fusion_cases.py and sweep_ref.full_union; back ends as tests/test_fusion_exact.py names them.
Every assertion is an equality."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import fusion_cases as fc
from tests import fusion_ref as fr
from tests import rank_ref
from tests import sweep_ref as sr

pytestmark = pytest.mark.gpu

A9 = sr.A9
# name -> (tile_docs, docs, forced quota); a case with a size of its own (depth_ge_n, full_union) keeps it
BACKENDS = {"one4096": (4096, fc.N_SMALL, None), "one8192": (8192, fc.N_TWO_TILES, None),
            "multi": (4096, fc.N_TWO_TILES, None), "round2": (4096, fc.N_TWO_TILES, 1)}
CASES = list(fc.EDGES) + list(fc.RANDOM) + ["full_union"]
E_INVAL, E_NODEVICE, E_RANGE = -1, -5, -8


@pytest.fixture(scope="module")
def m(built):
    import mllm_sparse_retrieval_amd as m

    return m


@functools.lru_cache(maxsize=None)
def _case(name, n):
    if name == "full_union":
        case, S, D = sr.full_union(n)
        for a in (S, D):
            a.setflags(write=False)
        return case, S, D
    return fc.get(name, n)


@functools.lru_cache(maxsize=None)
def _ref(name, n):
    """The whole union at every alpha of A9, computed once per case and left unchanged."""
    case, S, D = _case(name, n)
    out = sr.sweep(S, D, case["depth"], A9, case["self_ord"], 2 * case["depth"])
    for a in out:
        a.setflags(write=False)
    return out


def _prefix(full, k):
    """The first k columns of whole-union slices, padded the way the call pads."""
    ords, bits, cnt = full
    c = np.minimum(cnt, k).astype(np.int32)
    valid = np.arange(k)[None, None, :] < c[:, :, None]
    return np.where(valid, ords[:, :, :k], fr.PAD).astype(np.uint32), np.where(valid, bits[:, :, :k], 0).astype(np.uint32), c


def _precs(case):
    return ("f32", "fp16") if case["prec"] == "fp16" else ("f32",)


def _quota(monkeypatch, quota):
    if quota:
        monkeypatch.setenv("MSR_HYBRID_QUOTA", str(quota))
    else:
        monkeypatch.delenv("MSR_HYBRID_QUOTA", raising=False)


def _index(m, workdir, case, tile):
    n = len(case["r2o"])
    ids = ["%07d" % o for o in case["r2o"]]                    # doc ids = zero-padded ordinals: ordinal != row
    return m.build_index_from_csr(os.path.join(str(workdir), f"{case['name']}_{n}_{tile}.idx"),
                                  *rank_ref.docs_to_csr(case["Dm"]), case["Dm"].shape[1], doc_ids=ids, tile_docs=tile)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, "first differences at", bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def _same_lists(got, want, what):
    _same(got[2], want[2], what + ("counts",))
    _same(got[0], want[0], what + ("ordinals",))                # padding included: 0xFFFFFFFF
    _same(got[1].view(np.uint32), want[1].view(np.uint32), what + ("fused score bits",))   # padding included: +0


# ------------------------------------------------------------------------------------------ a. reference exactness
@pytest.mark.parametrize("backend", list(BACKENDS))
@pytest.mark.parametrize("name", CASES)
def test_reference_exact(m, tmp_path, monkeypatch, name, backend):
    from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_sweep

    tile, n, quota = BACKENDS[backend]
    _quota(monkeypatch, quota)
    case, S, D = _case(name, n)
    full = _ref(name, n)
    depth = case["depth"]
    qp, qt, qw = rank_ref.csr(case["queries"])
    path = _index(m, tmp_path, case, tile)
    with m.SparseIndex(path, device=0) as ix:
        for prec in _precs(case):
            dix = DenseIndex(case["p"], precision=prec)
            try:
                for k in sorted({min(k, 2 * depth) for k in (1, 10, 65, 2 * depth)}):
                    o, f, c, ms = hybrid_sweep(ix, dix, qp, qt, qw, case["q"], depth, k, A9, case["r2o"], case["self_ord"])
                    assert o.shape == f.shape == (len(A9), len(qp) - 1, k) and c.shape == (len(A9), len(qp) - 1)
                    assert ms["groups"] == 1 and ms["dense_select"] == 0, ms
                    _same_lists((o, f, c), _prefix(full, k), (name, backend, prec, k))
            finally:
                dix.close()
    if name == "full_union":
        assert (full[2] == 2 * sr.FULL_DEPTH).all()            # the sort ran at its capacity


# -------------------------------------------------------------------------- b. identities against the existing calls
@pytest.mark.parametrize("backend", ["one4096", "multi"])
@pytest.mark.parametrize("name", list(fc.RANDOM))
def test_identities(m, tmp_path, monkeypatch, name, backend):
    from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_search, hybrid_search_f32, hybrid_search_union, hybrid_sweep

    tile, n, _ = BACKENDS[backend]
    _quota(monkeypatch, None)
    case, S, D = _case(name, n)
    depth, r2o, so = case["depth"], case["r2o"], case["self_ord"]
    qp, qt, qw = rank_ref.csr(case["queries"])
    prec = case["prec"]
    topk = hybrid_search_f32 if prec == "f32" else hybrid_search
    path = _index(m, tmp_path, case, tile)
    with m.SparseIndex(path, device=0) as ix:
        dix = DenseIndex(case["p"], precision=prec)
        try:
            sw = {k: hybrid_sweep(ix, dix, qp, qt, qw, case["q"], depth, k, A9, r2o, so) for k in (10, 65, 2 * depth)}
            for a, alpha in enumerate(A9):
                for k in (10, 65):
                    o, f, c, ms = topk(ix, dix, qp, qt, qw, case["q"], depth, k, alpha, r2o, so)
                    fused = ms["fusion"] == 0                   # hybrid_tiles alone: one tile and k <= 64
                    assert fused == (backend == "one4096" and k == 10), (backend, k, ms)
                    _same_lists((sw[k][0][a], sw[k][1][a], sw[k][2][a]), (o, f, c), (name, backend, alpha, k, "top-k"))
                u = hybrid_search_union(ix, dix, qp, qt, qw, case["q"], depth, alpha, r2o, so, with_lists=False)
                for k in (10, 65, 2 * depth):
                    want = _prefix((u[0][None], u[1].view(np.uint32)[None], u[2][None]), k)
                    _same_lists((sw[k][0][a:a + 1], sw[k][1][a:a + 1], sw[k][2][a:a + 1]),
                                (want[0], want[1].view(np.float32), want[2]), (name, backend, alpha, k, "union"))
        finally:
            dix.close()


# ------------------------------------------------------------------------------------------------- c. independence
@pytest.fixture()
def random_multi(m, tmp_path, monkeypatch):
    """random_fp16 on two 4096-doc tiles with an f32 handle open: (ix, dix, call arguments, case)."""
    from mllm_sparse_retrieval_amd.dense import DenseIndex

    _quota(monkeypatch, None)
    case, S, D = _case("random_fp16", fc.N_TWO_TILES)
    path = _index(m, tmp_path, case, 4096)
    ix = m.SparseIndex(path, device=0)
    dix = DenseIndex(case["p"], precision="f32")
    yield ix, dix, rank_ref.csr(case["queries"]), case
    dix.close()
    ix.close()


def test_independent_of_the_other_alphas(random_multi):
    from mllm_sparse_retrieval_amd.dense import hybrid_sweep

    ix, dix, (qp, qt, qw), case = random_multi
    depth, k = case["depth"], 65
    call = lambda alphas: hybrid_sweep(ix, dix, qp, qt, qw, case["q"], depth, k, alphas, case["r2o"], case["self_ord"])  # noqa: E731
    base = call(A9)
    perm = [4, 8, 0, 4, 7, 2, 6, 1, 3, 5, 0]                    # a permutation of A9's positions plus two duplicates
    got = call([A9[i] for i in perm])
    _same_lists(got[:3], tuple(x[perm] for x in base[:3]), ("permuted",))
    for a in (0, 2, 8):                                         # n_alphas = 1
        one = call([A9[a]])
        assert one[3]["groups"] == 1
        _same_lists(one[:3], tuple(x[a:a + 1] for x in base[:3]), ("alone", a))
    grid64 = [A9[i % 9] if i % 7 == 0 else (i - 8) / 40 for i in range(64)]        # n_alphas = 64, A9's values among them
    full = call(grid64)
    assert full[0].shape == (64, len(qp) - 1, k)
    for i in range(0, 64, 7):
        _same_lists(tuple(x[i:i + 1] for x in full[:3]), tuple(x[i % 9:i % 9 + 1] for x in base[:3]), ("of 64", i))
    ref = _prefix(sr.sweep(*_case("random_fp16", fc.N_TWO_TILES)[1:], depth, [grid64[9], grid64[63]], case["self_ord"], k), k)
    _same_lists((full[0][[9, 63]], full[1][[9, 63]], full[2][[9, 63]]), (ref[0], ref[1].view(np.float32), ref[2]), ("64 vs ref",))


# ------------------------------------------------------------------------------------------------------- d. groups
def test_alpha_groups(m, tmp_path, monkeypatch):
    """64 alphas x 257 queries x k = 2048: 64 * 257 * 2048 * 8 B = 257 MiB of lists, one MiB more than one staging group
    holds (256 MiB), every query with exactly 2048 members."""
    from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_sweep

    _quota(monkeypatch, None)
    nq, k = 257, 2 * sr.FULL_DEPTH
    assert 64 * nq * k * 8 > (256 << 20) >= 64 * (nq - 1) * k * 8
    case, S, D = sr.full_union(sr.N_FULL_MIN, nq=nq, seed=1)
    alphas = [i / 63 for i in range(64)]
    qp, qt, qw = rank_ref.csr(case["queries"])
    path = _index(m, tmp_path, case, 4096)
    with m.SparseIndex(path, device=0) as ix:
        dix = DenseIndex(case["p"], precision="f32")
        try:
            call = lambda al: hybrid_sweep(ix, dix, qp, qt, qw, case["q"], sr.FULL_DEPTH, k, al, case["r2o"], None)  # noqa: E731
            o, f, c, ms = call(alphas)
            assert ms["groups"] > 1, ms
            assert (c == k).all()
            for g in range(4):
                po, pf, pc, pms = call(alphas[16 * g:16 * g + 16])
                assert pms["groups"] == 1
                _same_lists((o[16 * g:16 * g + 16], f[16 * g:16 * g + 16], c[16 * g:16 * g + 16]), (po, pf, pc), ("four calls", g))
        finally:
            dix.close()
    qs, al = [0, 100, 256], [0, 31, 63]                         # a sample of queries, alphas of both groups
    ref = sr.sweep(S[qs], D[qs], sr.FULL_DEPTH, [alphas[a] for a in al], None, k)
    _same_lists((o[al][:, qs], f[al][:, qs], c[al][:, qs]), (ref[0], ref[1].view(np.float32), ref[2]), ("reference",))


# ------------------------------------------------------------------------------------------------- e. steady state
def test_second_call_allocates_nothing(random_multi):
    from mllm_sparse_retrieval_amd.dense import hybrid_sweep

    ix, dix, (qp, qt, qw), case = random_multi
    call = lambda: hybrid_sweep(ix, dix, qp, qt, qw, case["q"], case["depth"], 65, A9, case["r2o"], case["self_ord"])  # noqa: E731
    first = call()
    before = dix.stats()
    second = call()
    assert dix.stats() == before and before["device_allocs"] > 0
    _same_lists(second[:3], first[:3], ("repeat",))


# --------------------------------------------------------------------------------------------- f. misuse and edges
def _raw(L, ix_h, dx_h, qp, qt, qw, q, is_f32, nq, depth, k, alphas, n_alphas, r2o, so, ords, sc, n, ms):
    from mllm_sparse_retrieval_amd._cabi import ptr

    return L.msr_hybrid_sweep(ix_h, dx_h, ptr(qp), ptr(qt), ptr(qw), ptr(q), is_f32, nq, depth, k, ptr(alphas), n_alphas, 1,
                              ptr(r2o), ptr(so), ptr(ords), ptr(sc), ptr(n), ms)


def test_refusals(m, tmp_path, random_multi):
    from mllm_sparse_retrieval_amd import _cabi
    from mllm_sparse_retrieval_amd.dense import DenseIndex, _as_fp16_rows

    ix, dix, (qp, qt, qw), case = random_multi
    L = _cabi.lib()
    nq, depth, k = len(qp) - 1, 8, 16
    q = np.ascontiguousarray(case["q"], dtype=np.float32)
    q16 = _as_fp16_rows(q).view(np.uint16)                      # (columns padded to the fp16 handle's multiple of 32)
    al = np.array([0.0, 0.5], np.float32)
    r2o = np.ascontiguousarray(case["r2o"], dtype=np.uint32)
    ords, sc, n = np.zeros((2, nq, k), np.uint32), np.zeros((2, nq, k), np.float32), np.zeros((2, nq), np.int32)
    ms = (ctypes.c_float * 6)()
    good = dict(ix_h=ix._h, dx_h=dix._h, qp=qp, qt=qt, qw=qw, q=q, is_f32=1, nq=nq, depth=depth, k=k, alphas=al, n_alphas=2,
                r2o=r2o, so=None, ords=ords, sc=sc, n=n, ms=ms)
    rc = lambda **kw: _raw(L, **{**good, **kw})  # noqa: E731
    assert rc() == 0
    nan, inf = np.array([0.0, np.nan], np.float32), np.array([np.inf, 0.5], np.float32)
    nan65 = np.full(65, np.nan, np.float32)
    for kw in (dict(ix_h=None), dict(dx_h=None), dict(qp=None), dict(alphas=None), dict(r2o=None), dict(ords=None),
               dict(sc=None), dict(n=None), dict(q=None), dict(nq=-1), dict(is_f32=0, q=q16), dict(alphas=nan), dict(alphas=inf),
               dict(alphas=nan, depth=0), dict(alphas=nan65, n_alphas=65, k=0)):             # INVAL comes before RANGE
        assert rc(**kw) == E_INVAL, kw
        assert b"msr_hybrid_sweep" in L.msr_last_error(), kw
    for kw in (dict(depth=0), dict(depth=1025, k=1), dict(k=0), dict(k=2 * depth + 1), dict(n_alphas=0), dict(n_alphas=-3),
               dict(n_alphas=65, alphas=np.zeros(65, np.float32))):
        assert rc(**kw) == E_RANGE, kw
    # a handle without a device: RANGE still comes first, then NODEVICE
    path = _index(m, tmp_path, case, 4096)
    with m.SparseIndex(path, device=-1) as host_ix:
        assert rc(ix_h=host_ix._h, depth=0) == E_RANGE
        assert rc(ix_h=host_ix._h) == E_NODEVICE
    # handles the union pass does not serve
    with m.SparseIndex(path, device=0, shard=0, n_shards=2) as shard:
        assert rc(ix_h=shard._h) == E_INVAL and b"shard" in L.msr_last_error()
    with m.SparseIndex(path, device=0, term_shard=(0, 2)) as tshard:
        assert rc(ix_h=tshard._h) == E_INVAL and b"shard" in L.msr_last_error()
    big = _index(m, tmp_path, case, 12288)
    with m.SparseIndex(big, device=0) as ix12:
        assert rc(ix_h=ix12._h) == E_INVAL and b"12288" in L.msr_last_error()
        assert rc(ix_h=ix12._h, depth=0) == E_INVAL                                           # INVAL before RANGE
    f16 = DenseIndex(case["p"], precision="fp16")
    try:
        assert rc(dx_h=f16._h) == E_INVAL                                                     # f32 queries, fp16 handle
        assert rc(dx_h=f16._h, is_f32=0, q=q16) == 0
    finally:
        f16.close()
    # nq == 0: MSR_OK, nothing launched, nothing allocated
    before = dix.stats()
    assert rc(nq=0, qp=np.zeros(1, np.int64), q=None) == 0 and [ms[i] for i in range(6)] == [0.0] * 6
    assert dix.stats() == before


def test_empty_batch_through_python(random_multi):
    from mllm_sparse_retrieval_amd.dense import hybrid_sweep

    ix, dix, _, case = random_multi
    o, f, c, ms = hybrid_sweep(ix, dix, [0], [], [], np.zeros((0, case["q"].shape[1]), np.float32), 8, 16, A9, case["r2o"])
    assert o.shape == f.shape == (9, 0, 16) and c.shape == (9, 0) and ms["groups"] == 0


def test_named_edges(m, tmp_path, monkeypatch):
    """A query with no sparse term (short_lists, query 1: dense members only, as many as the depth) and a query whose
    self_ord heads both lists (self_extremes, query 4: no remaining member is at 1 on either side, at any alpha)."""
    from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_sweep

    _quota(monkeypatch, None)
    for name, qi in (("short_lists", 1), ("self_extremes", 4)):
        case, S, D = _case(name, fc.N_TWO_TILES)
        full = _ref(name, fc.N_TWO_TILES)
        depth = case["depth"]
        qp, qt, qw = rank_ref.csr(case["queries"])
        with m.SparseIndex(_index(m, tmp_path, case, 4096), device=0) as ix:
            dix = DenseIndex(case["p"], precision="f32")
            try:
                got = hybrid_sweep(ix, dix, qp, qt, qw, case["q"], depth, 2 * depth, A9, case["r2o"], case["self_ord"])
            finally:
                dix.close()
        _same_lists(got[:3], (full[0], full[1].view(np.float32), full[2]), (name,))
        if name == "short_lists":
            assert len(case["queries"][qi]) == 0 and (got[2][:, qi] == depth).all()
            assert (got[1][A9.index(0.0), qi] == 0).all()      # alpha = 0: only the (empty) sparse side has weight
        else:
            so = int(case["self_ord"][qi])
            assert so == int(np.argmax(S[qi])) and (got[0][:, qi] != so).all()
            a = A9.index(0.5)
            assert got[1][a, qi].max() < np.float32(1.0)       # the doc that was at 1 + 1 is the one taken out


# ---------------------------------------------------------------------------------------------------------- g. CLI
N_QUERIES = 300


@pytest.fixture(scope="module")
def flickr_encode(m, tmp_path_factory):
    from mllm_sparse_retrieval_amd import cli

    root = tmp_path_factory.mktemp("cli_sweep")
    enc, dense = str(root / "enc"), str(root / "dense")
    cli.main(["encode", "--synthetic", "flickr", "--n_images", "2000", "--sparse_output_dir", enc, "--threads", "4",
              "--dense_output_dir", dense, "--dense_dim", "64"])
    cli.main(["index", "--input", enc, "--threads", "4", "--impact", "--pretokenized"])
    with open(os.path.join(enc, "query.tsv")) as f, open(root / "queries.tsv", "w") as g:
        g.writelines(f.readlines()[:N_QUERIES])
    return root, enc, dense, str(root / "queries.tsv")


def _read(path):
    with open(path) as f:
        return f.read()


@pytest.mark.parametrize("prec", ["fp16", "f32"])
def test_cli_sweep_against_plain_runs(m, flickr_encode, capsys, monkeypatch, prec):
    from mllm_sparse_retrieval_amd import cli

    _quota(monkeypatch, None)
    root, enc, dense, queries = flickr_encode
    common = ["search", "--sparse_index", enc, "--passage_reps", dense, "--depth", "100", "--remove_query", "--query_type", "text",
              "--dataset_name", "flickr", "--quiet", "--queries", queries, "--qrels", os.path.join(enc, "qrels.csv"),
              *(["--hybrid_f32"] if prec == "f32" else [])]
    grid = ["0", "0.3", "1"]

    def run(name, *extra):
        capsys.readouterr()
        out_dir = str(root / f"{name}_{prec}")
        cli.main([*common, "--save_dir", out_dir, *extra])
        return out_dir, capsys.readouterr().out.splitlines()

    plain = {}
    for a in grid:
        out_dir, lines = run(f"plain_{a}", "--alpha", a)
        recall = [ln for ln in lines if ln.startswith("Fusion/Hybrid reps recall: ")]
        assert len(recall) == 1
        plain[a] = (out_dir, recall[0].split(": ", 1)[1], lines)
    sweep_dir, lines = run("sweep", "--alpha", "0.3", "--alphas", ",".join(grid), "--sweep_runs")
    swept = [ln for ln in lines if ln.startswith("Fusion/Hybrid sweep alpha ")]
    assert swept == [f"Fusion/Hybrid sweep alpha {a}: {plain[a][1]}" for a in grid]
    assert [ln for ln in lines if not ln.startswith("Fusion/Hybrid sweep alpha ")] == plain["0.3"][2]    # the usual report
    want_tsv = "".join("\t".join([a] + [x.split(" ", 1)[1] for x in plain[a][1].split(", ")]) + "\n" for a in grid)
    assert _read(os.path.join(sweep_dir, "fusion.sweep.tsv")) == want_tsv
    for name in ("fusion.trec", "sparse.trec", "dense.trec"):
        assert _read(os.path.join(sweep_dir, name)) == _read(os.path.join(plain["0.3"][0], name)), name
    for a in grid:
        assert _read(os.path.join(sweep_dir, f"fusion.alpha_{a}.trec")) == _read(os.path.join(plain[a][0], "fusion.trec")), a
    assert len({_read(os.path.join(plain[a][0], "fusion.trec")) for a in grid}) == 3         # the alphas differ
    # --fusion_only is honoured: the same sweep lines, no sparse or dense report
    only_dir, lines = run("sweep_only", "--alpha", "0.3", "--alphas", ",".join(grid), "--fusion_only")
    assert [ln for ln in lines if ln.startswith("Fusion/Hybrid sweep alpha ")] == swept
    assert not any(ln.startswith(("Sparse reps recall", "Dense reps recall")) for ln in lines)
    assert _read(os.path.join(only_dir, "fusion.sweep.tsv")) == want_tsv
