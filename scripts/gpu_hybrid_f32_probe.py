"""f32 hybrid search (msr_hybrid_search_f32) at the reference's two hybrid shapes, H = 4096, depth 1000, alpha 0.5 (GPU):

  (a) i2t, the run of scripts/search.sh: 5 000 image queries x 25 010 caption docs, --remove_query, fused top-1000
      (four tiles: the multi-tile candidate kernels);
  (b) t2i: 25 010 caption queries x 5 000 image docs, fused top-10 (one tile: the single-tile fused kernel).

Unit rows (random, f32, not rounded to fp16), the sparse side of workloads.hybrid_vectors. Per shape: one warm-up call,
then --reps timed calls of hybrid_search_f32 over the whole query matrix; the kernel ms from the library's device events
(ms[4] of the last call), host-inclusive ms (wall clock around the call), the GEMM ms of msr_dense_search_f32 at the same
shape (depth 1000, same handle), the fp16 hybrid (hybrid_search on an fp16 handle) at the same shape, and the agreement
of the fused top-k ids between f32 and fp16 (slot by slot). One JSON line on stdout. Kernel times without the events:
run this under rocprofv3 --kernel-trace --stats.

    python scripts/gpu_hybrid_f32_probe.py [--reps 3] [--out profiles/hybrid_f32_probe.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mllm_sparse_retrieval_amd as m  # noqa: E402
from mllm_sparse_retrieval_amd import workloads  # noqa: E402
from mllm_sparse_retrieval_amd.dense import DenseIndex, hybrid_search, hybrid_search_f32, row_to_ordinal  # noqa: E402

H, DEPTH, ALPHA, N_TERMS = 4096, 1000, 0.5, 30000


def timed(fn, reps):
    fn()  # warm-up: ordinal rows, scratch, first launches
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        walls.append((time.perf_counter() - t0) * 1e3)
    return out, walls


def shape(n, nq, k, remove, reps, tmp):
    docs, (qp, qt, qw), p, q = workloads.hybrid_vectors(n, nq, H, N_TERMS)
    path = m.build_index_from_csr(os.path.join(tmp, f"h{n}.idx"), *docs, N_TERMS)
    rec = dict(n=n, nq=nq, k=k, remove_query=remove)
    with m.SparseIndex(path, device=0) as ix:
        r2o = row_to_ordinal(ix, [str(i) for i in range(n)])
        self_ord = r2o[:nq].astype(np.int32) if remove else None
        res = {}
        for prec, fn in (("f32", hybrid_search_f32), ("fp16", hybrid_search)):
            dix = DenseIndex(p, device=0, precision=prec)
            try:
                (ords, fs, cnt, ms), walls = timed(lambda: fn(ix, dix, qp, qt, qw, q, DEPTH, k, ALPHA, r2o, self_ord), reps)
                res[prec] = ords
                r = dict(kernel_ms={a: round(b, 3) for a, b in ms.items()}, kernel_ms_sum=round(sum(ms.values()), 3),
                         host_inclusive_ms=round(min(walls), 3), host_inclusive_ms_all=[round(w, 3) for w in walls])
                if prec == "f32":
                    timed(lambda: dix.search(q, DEPTH), 1)  # (the GEMM lap of the last call)
                    r["dense_search_f32_gemm_ms"] = round(dix.last_ms[0], 3)
                    r["hybrid_gemm_over_dense_search_gemm"] = round(ms["dense_gemm"] / dix.last_ms[0], 3)
                rec[prec] = r
            finally:
                dix.close()
        rec[f"top{k}_id_agreement_f32_vs_fp16"] = float((res["f32"] == res["fp16"]).mean())
    os.remove(path)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    a = ap.parse_args()
    rec = dict(probe="hybrid_f32", h=H, depth=DEPTH, alpha=ALPHA, shapes={})
    with tempfile.TemporaryDirectory(prefix="msr_hf32_") as tmp:
        rec["shapes"]["a_i2t_5000q_x_25010d_k1000"] = shape(25010, 5000, 1000, True, a.reps, tmp)
        rec["shapes"]["b_t2i_25010q_x_5000d_k10"] = shape(5000, 25010, 10, False, a.reps, tmp)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
