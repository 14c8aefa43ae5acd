"""f32 dense search, host side: the fmaf-chain emulator the GPU tests compare against equals libm's fmaf, the
dense-only `search` command checks its arguments before touching a GPU, and msr_dense_open_f32 has no CPU path."""
import ctypes
import ctypes.util
import pickle

import numpy as np
import pytest

from tests.f32_chain import chain_scores, f32_keys, fmaf, topk


@pytest.fixture(scope="module")
def libm_fmaf():
    name = ctypes.util.find_library("m") or "libm.so.6"
    f = ctypes.CDLL(name).fmaf
    f.restype = ctypes.c_float
    f.argtypes = [ctypes.c_float] * 3
    return f


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def _random_triples(rng, n):
    def f32(size, lo, hi):
        mant = rng.uniform(1.0, 2.0, size)
        return (rng.choice([-1.0, 1.0], size) * mant * np.exp2(rng.integers(lo, hi, size))).astype(np.float32)

    a, b = f32(n, -30, 30), f32(n, -30, 30)
    c = f32(n, -60, 60)
    sel = rng.integers(0, 4, n)
    # cancellation: c close to -a*b; zero; subnormal products and accumulators
    ab = (a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)
    c = np.where(sel == 1, -ab * np.float32(1 + 2.0 ** -20), c)
    c = np.where(sel == 2, np.float32(0), c)
    tiny = sel == 3
    a = np.where(tiny, f32(n, -80, -70), a)
    b = np.where(tiny, f32(n, -80, -70), b)
    c = np.where(tiny, f32(n, -150, -126), c)
    return a.astype(np.float32), b.astype(np.float32), c.astype(np.float32)


def _midpoint_triples(rng, n):
    """x = c + ulp(c)/2 - tiny: float64 rounds the exact value onto the f32 midpoint, round-to-even would go to the
    wrong neighbour whenever c's last mantissa bit is 1. a * b = half * (1 - d^2) exactly, d = t * 2^-23."""
    c = (rng.uniform(1.0, 2.0, n) * np.exp2(rng.integers(-40, 40, n))).astype(np.float32)
    c = np.where(rng.integers(0, 2, n) == 1, -c, c).astype(np.float32)
    half_e = np.frexp(np.abs(c).astype(np.float64))[1] - 25  # |c| in [2^(E-1), 2^E): ulp/2 = 2^(E-25)
    t = rng.integers(1, 9, n).astype(np.float64)
    d = t * 2.0 ** -23
    sgn = np.sign(c.astype(np.float64))
    a = (sgn * np.exp2(np.floor(half_e / 2)) * (1 + d)).astype(np.float32)
    b = (np.exp2(half_e - np.floor(half_e / 2)) * (1 - d)).astype(np.float32)
    return a, b, c


def test_emulator_equals_libm_fmaf(libm_fmaf):
    rng = np.random.default_rng(5)
    a, b, c = _random_triples(rng, 100_000)
    a2, b2, c2 = _midpoint_triples(rng, 20_000)
    a, b, c = np.concatenate([a, a2]), np.concatenate([b, b2]), np.concatenate([c, c2])
    got = fmaf(a, b, c)
    want = np.array([libm_fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], dtype=np.float32)
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, [(a[i], b[i], c[i], got[i], want[i]) for i in bad[:5]]
    # the midpoint family does exercise the correction: plain float64 rounding differs there
    plain = (a2.astype(np.float64) * b2.astype(np.float64) + c2.astype(np.float64)).astype(np.float32)
    assert (_bits(plain) != _bits(fmaf(a2, b2, c2))).sum() > 1000


def test_constructed_midpoint():
    # 2^30 + 128 + (64 - 2^-40): float64 gives 2^30 + 192, the midpoint whose even neighbour is 2^30 + 256
    a, b, c = np.float32(8 * (1 + 2.0 ** -23)), np.float32(8 * (1 - 2.0 ** -23)), np.float32(2.0 ** 30 + 128)
    assert float(fmaf(a, b, c)) == 2.0 ** 30 + 128
    assert float(fmaf(-a, b, -c)) == -(2.0 ** 30 + 128)


def test_chain_and_topk_conventions():
    q = np.array([[1.0, 2.0, 0.0], [-1.0, 0.0, 0.0]], np.float32)
    p = np.array([[1.0, 1.0, 5.0], [3.0, 0.0, 0.0], [0.0, 0.0, 0.0], [-3.0, 0.0, 0.0]], np.float32)
    s = chain_scores(q, p)
    assert s.tolist() == [[3.0, 3.0, 0.0, -3.0], [-1.0, -3.0, 0.0, 3.0]]
    assert not np.signbit(s[0, 2])  # +0 start: zero products keep +0
    idx, key, n = topk(s, 6)
    assert idx[0, :4].tolist() == [0, 1, 2, 3]  # tie 3.0 / 3.0: lower row first
    assert idx[1, :4].tolist() == [3, 2, 0, 1]
    assert (idx[:, 4:] == 0xFFFFFFFF).all() and (key[:, 4:] == 0).all() and n.tolist() == [4, 4]
    assert (np.diff(f32_keys(np.array([-2.0, -0.0, 0.0, 1e-45, 1.0], np.float32)).astype(np.int64)) > 0).all()


def test_search_argument_checks(tmp_path, capsys):
    from mllm_sparse_retrieval_amd.cli import main

    with pytest.raises(SystemExit) as e:
        main(["search", "--depth", "10"])
    assert "--passage_reps" in str(e.value) and "--sparse_index" in str(e.value)
    with open(tmp_path / "corpus_0.pkl", "wb") as f:
        pickle.dump((np.zeros((4, 8), np.float32), ["a", "b", "c", "d"]), f)
    for depth in (1025, 0):
        with pytest.raises(SystemExit) as e:
            main(["search", "--passage_reps", str(tmp_path), "--depth", str(depth)])
        assert "MSR_KMAX" in str(e.value)


def test_search_help_documents_dense_only(capsys):
    from mllm_sparse_retrieval_amd.cli import main

    with pytest.raises(SystemExit):
        main(["search", "--help"])
    out = " ".join(capsys.readouterr().out.split())
    assert "dense-only" in out and "ignored by the sparse and hybrid routes" in out


def test_open_f32_without_device(built):
    from mllm_sparse_retrieval_amd import _cabi
    from mllm_sparse_retrieval_amd._cabi import NoDeviceError
    from mllm_sparse_retrieval_amd.dense import DenseIndex

    L = _cabi.lib()
    p = np.ones((5, 3), np.float32)
    h = ctypes.c_void_p()
    assert L.msr_dense_open_f32(_cabi.ptr(p), 5, 3, -1, ctypes.byref(h)) == -5  # MSR_E_NODEVICE
    assert not h.value
    assert L.msr_dense_open_f32(_cabi.ptr(p), 5, 0, -1, ctypes.byref(h)) == -1  # h = 0: MSR_E_INVAL
    assert L.msr_dense_open_f32(None, 5, 3, -1, ctypes.byref(h)) == -1          # rows missing: MSR_E_INVAL
    with pytest.raises(NoDeviceError):
        DenseIndex(p, device=-1, precision="f32")
    with pytest.raises(ValueError):
        DenseIndex(p, device=-1, precision="bf16")
