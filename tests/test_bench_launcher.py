"""bench.py's own launcher (CPU, gloo): `--gpus N` without a launcher must start N ranks itself and relay rank 0's
line; a box with fewer GPUs than ranks, or a WORLD_SIZE that contradicts --gpus, must end non-zero — never a silent
1-GPU measurement reported as N (reference launcher: deepspeed --num_gpus=4, scripts/search_sparse.sh:14)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env=None, timeout=300):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, BENCH] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e,
                          timeout=timeout)


def test_launcher_starts_n_ranks_and_relays_one_json_line():
    p = _run(["--gpus", "2", "--launcher-selftest"])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out == {"launcher_selftest": True, "n_gpus": 2, "max_rank_seen": 1}


def test_more_ranks_than_gpus_is_refused():
    import torch

    n_dev = torch.cuda.device_count()
    p = _run(["--gpus", str(n_dev + 2), "--steps", "1", "--warmup", "0", "--no-c4", "--no-c5", "--no-c3", "--no-cpu"])
    assert p.returncode == 2
    assert b"HIP device(s) are visible" in p.stderr and p.stdout.strip() == b""


def test_world_size_mismatch_is_refused():
    p = _run(["--gpus", "4", "--launcher-selftest"], env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode == 2 and b"WORLD_SIZE=1" in p.stderr


def test_bad_step_counts_and_orphan_selectors_are_refused():
    for args in (["--steps", "0"], ["--warmup", "-1"], ["--only-c4"], ["--full", "--only-c3", "--dump-outputs", "x"]):
        p = _run(args)
        assert p.returncode == 2 and b"error:" in p.stderr and p.stdout.strip() == b"", args


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_dumps_its_last_step(built, tmp_path):
    """A plain run prints the headline figure without what needs runs of its own (that is --full's); --dump-outputs
    writes the results of its last timed step, which on the seeded headline workload are the oracle's."""
    import numpy as np

    from mllm_sparse_retrieval_amd import workloads
    from tests import helpers

    p = _run(["--steps", "3", "--warmup", "1", "--flickr-images", "3000", "--dump-outputs", str(tmp_path)])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    line = json.loads(p.stdout.decode().strip().splitlines()[-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["unit"] == "queries/s" and line["dtype"] == "u32"
    nq = line["config"]["queries_per_step_per_gpu"]
    assert line["value"] == pytest.approx(nq / (line["ms_per_step"] * 1e-3), rel=1e-3)
    assert not {"roofline", "recall", "cpu_baseline", "host_inclusive", "c3_coco5k", "c4_1m", "c5_hybrid"} & set(line)
    got = {name: np.load(tmp_path / f"{name}.npy") for name in ("doc_ids", "scores", "scores_exact", "n_hits")}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    wl = workloads.flickr30k_t2i(n_images=3000, seed=1, threads=8)
    oix, order = helpers.taat_oracle(wl.docs, wl.n_terms)
    w_ord, w_sc, w_n = oix.search(*wl.queries, wl.k, threads=16)
    assert len(got["n_hits"]) == nq == len(w_n) and (got["n_hits"] == w_n).all()
    mask = np.arange(wl.k)[None, :] < w_n[:, None]
    assert (got["doc_ids"][mask] == order[w_ord[mask]]).all() and (got["doc_ids"][~mask] == -1).all()
    assert (got["scores_exact"][mask] == w_sc[mask]).all()
    assert (got["scores"][mask] == w_sc[mask].astype(np.float32)).all()
