"""search --hybrid_f32 and hybrid_search_f32, host side: the argument refusals that need no index and no GPU, the help
text, the precision checks of both hybrid entry points, and the new C-ABI symbol bound."""
from types import SimpleNamespace

import numpy as np
import pytest


def _search(*args):
    from mllm_sparse_retrieval_amd.cli import main

    with pytest.raises(SystemExit) as e:
        main(["search", *args])
    return str(e.value)


def test_hybrid_f32_refused_with_use_gpu(tmp_path):
    msg = _search("--sparse_index", str(tmp_path), "--passage_reps", str(tmp_path), "--hybrid_f32", "--use_gpu")
    assert "--hybrid_f32" in msg and "--use_gpu" in msg


@pytest.mark.parametrize("which", ["--sparse_index", "--passage_reps"])
def test_hybrid_f32_needs_both_sides(tmp_path, which):
    msg = _search(which, str(tmp_path), "--hybrid_f32")
    assert "--hybrid_f32" in msg and "--passage_reps" in msg and "--sparse_index" in msg


def test_hybrid_f32_defaults_off():
    from mllm_sparse_retrieval_amd.cli import _check_search_args

    # a namespace without the attribute (callers that build their own) and the flag off both pass
    _check_search_args(SimpleNamespace(sparse_index="x", passage_reps="y", depth=1000, use_gpu=True))
    _check_search_args(SimpleNamespace(sparse_index="x", passage_reps="y", depth=1000, use_gpu=True, hybrid_f32=False))


def test_help_documents_hybrid_f32(capsys):
    from mllm_sparse_retrieval_amd.cli import main

    with pytest.raises(SystemExit):
        main(["search", "--help"])
    out = " ".join(capsys.readouterr().out.split())
    assert "--hybrid_f32" in out and "msr_hybrid_search_f32" in out and "--host_fusion" in out


def test_precision_checks_before_any_device_call():
    from mllm_sparse_retrieval_amd.dense import hybrid_search, hybrid_search_f32

    q = np.zeros((1, 8), np.float32)
    r2o = np.zeros(1, np.uint32)
    with pytest.raises(ValueError, match="hybrid_search"):
        hybrid_search_f32(None, SimpleNamespace(precision="fp16", dim=8, n=1), [0, 0], [], [], q, 1, 1, 0.5, r2o)
    with pytest.raises(ValueError, match="hybrid_search_f32"):
        hybrid_search(None, SimpleNamespace(precision="f32", dim=8, n=1), [0, 0], [], [], q, 1, 1, 0.5, r2o)


def test_symbol_bound(built):
    from mllm_sparse_retrieval_amd import _cabi

    assert "msr_hybrid_search_f32" in {name for name, _, _ in _cabi.SYMBOLS}
    assert _cabi.lib().msr_hybrid_search_f32.restype is not None
