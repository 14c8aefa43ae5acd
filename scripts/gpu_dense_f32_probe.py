"""f32 flat dense search at the reference's two dense shapes, H = 4096, depth 10 (GPU):

  (a) scripts/search_dense.sh: 5 000 image queries x 25 010 caption passages (--query_type image);
  (b) the reverse: 25 010 caption queries x 5 000 image passages.

Unit rows (random, f32, not rounded to fp16). Per shape and precision: one warm-up call, then --reps timed calls of
DenseIndex.search over the whole query matrix; GEMM and select ms from the library's device events (last call),
host-inclusive ms (wall clock around the call: query upload from pageable memory, kernels, download), GEMM TFLOP/s
= 2 nq n H / GEMM time, its share of the f32 MFMA peak, and the largest |score - float64 score| over a sample of
queries. One JSON line on stdout. Kernel times without the events: run this under rocprofv3 --kernel-trace --stats.

    python scripts/gpu_dense_f32_probe.py [--reps 3] [--out profiles/dense_f32_probe.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mllm_sparse_retrieval_amd.dense import DenseIndex  # noqa: E402

F32_PEAK_TF = 157.3  # v_mfma_f32_32x32x2_f32: 64 FLOP / clk / SIMD x 4 SIMD x 256 CU x 2.4 GHz
H = 4096
DEPTH = 10


def unit_rows(rng, n, h):
    x = rng.standard_normal((n, h), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x


def measure(p, q, precision, reps, sample):
    dix = DenseIndex(p, device=0, precision=precision)
    try:
        dix.search(q, DEPTH)  # warm-up: scratch, first launches
        walls = []
        for _ in range(reps):
            t0 = time.perf_counter()
            s, i = dix.search(q, DEPTH)
            walls.append((time.perf_counter() - t0) * 1e3)
        gemm_ms, select_ms = dix.last_ms
    finally:
        dix.close()
    s64 = np.einsum("qh,qkh->qk", q[sample].astype(np.float64), p[i[sample]].astype(np.float64))
    flop = 2.0 * q.shape[0] * p.shape[0] * p.shape[1]
    return dict(gemm_ms=round(gemm_ms, 3), select_ms=round(select_ms, 3), host_inclusive_ms=round(min(walls), 3),
                host_inclusive_ms_all=[round(w, 3) for w in walls], gemm_tflops=round(flop / gemm_ms / 1e9, 2),
                max_abs_err_vs_f64=float(np.abs(s[sample] - s64).max())), i


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    a = ap.parse_args()
    rng = np.random.default_rng(2024)
    img, cap = unit_rows(rng, 5000, H), unit_rows(rng, 25010, H)
    rec = dict(probe="dense_f32", h=H, depth=DEPTH, f32_peak_tflops=F32_PEAK_TF, shapes={})
    for name, q, p in (("a_search_dense_i2t_5000x25010", img, cap), ("b_t2i_25010x5000", cap, img)):
        sample = rng.choice(q.shape[0], 64, replace=False)
        f32, i32 = measure(p, q, "f32", a.reps, sample)
        f16, i16 = measure(p, q, "fp16", a.reps, sample)
        f32["peak_share"] = round(f32["gemm_tflops"] / F32_PEAK_TF, 3)
        rec["shapes"][name] = dict(nq=q.shape[0], n=p.shape[0], tflop=round(2.0 * q.shape[0] * p.shape[0] * H / 1e12, 3),
                                   f32=f32, fp16=f16, top10_id_agreement_f32_vs_fp16=float((i32 == i16).mean()))
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
