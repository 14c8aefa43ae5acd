"""What exact ranks cost on the dense route (msr_dense_rank_rows) next to the f32 flat search of the same batch (GPU).

The reference's dense shape (scripts/search_dense.sh on COCO-5K i->t): 5 000 queries x 25 010 rows x H 4096, f32, five
listed rows per query. One warm-up and --reps timed repetitions each, in one process, of
  - DenseIndex.rank_rows: ms[0] (query upload + GEMM), ms[1] (the count kernel), host-inclusive wall time;
  - DenseIndex.search_keys at depth 10 and 1000: gemm_ms (GEMM, upload not included), select_ms (select + merge), wall.
All kernel figures are the library's HIP-event times, every repetition's min / median / max reported. Also checked: on
a sample of the queries every listed row with rank <= 1000 sits at column rank - 1 of the depth-1000 search with the
same key, and every other one is absent from it.

One JSON line on stdout, appended to --out if given.

    python scripts/gpu_dense_rank_probe.py [--reps 7] [--out profiles/dense_rank_probe.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mllm_sparse_retrieval_amd.dense import DenseIndex

    rng = np.random.default_rng(1)
    n, nq, h, nt = 25010, 5000, 4096, 5
    p = rng.standard_normal((n, h), dtype=np.float32)
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    q = rng.standard_normal((nq, h), dtype=np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t_ptr = np.arange(nq + 1, dtype=np.int64) * nt
    t_row = rng.integers(0, n, size=nq * nt).astype(np.uint32)
    out = dict(shape=dict(rows=n, queries=nq, h=h, targets_per_query=nt, precision="f32"), reps=a.reps)
    dix = DenseIndex(p, device=0, precision="f32")
    try:
        calls = (("rank_rows", lambda: dix.rank_rows(q, t_ptr, t_row), ("upload_gemm_ms", "count_ms")),
                 ("search_k10", lambda: dix.search_keys(q, 10), ("gemm_ms", "select_ms")),
                 ("search_k1000", lambda: dix.search_keys(q, 1000), ("gemm_ms", "select_ms")))
        for name, fn, labels in calls:
            fn()  # warm-up
            rows = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                fn()
                wall = (time.perf_counter() - t0) * 1e3
                ms = dix.last_rank_ms if name == "rank_rows" else dix.last_ms
                rows.append((ms[0], ms[1], wall))
            r = np.array(rows)
            out[name] = {lab: dict(min=float(r[:, j].min()), median=float(np.median(r[:, j])), max=float(r[:, j].max()))
                         for j, lab in enumerate(labels + ("wall_ms",))}
        idx, key, _ = dix.search_keys(q, 1000)
        ranks, keys = dix.rank_rows(q, t_ptr, t_row)
        ok = True
        for i in range(0, nq, 37):
            for e in range(i * nt, (i + 1) * nt):
                r, t = int(ranks[e]), int(t_row[e])
                ok &= bool(idx[i, r - 1] == t and key[i, r - 1] == keys[e]) if r <= 1000 else (t not in idx[i])
        out["link_ok"] = bool(ok)
    finally:
        dix.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    if not out["link_ok"]:
        sys.exit("rank_rows and search_keys disagree")


if __name__ == "__main__":
    main()
