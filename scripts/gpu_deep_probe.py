"""What deep lists cost (msr_search_deep, msr_dense_search_deep) next to the staged search of the same batch (GPU).

Shapes:
  coco5k_i2t      the reference's hybrid shape: 25 010 docs x 5 000 queries; sparse (120-term image queries), dense f32 and
                  dense fp16 (H 4096), each at k = 1 000, 2 000 and 16 384;
  flickr30k_t2i   the headline batch: 31 014 docs x 155 070 caption queries, sparse, k = 2 000.
Per (shape, route, k), one warm-up and --reps timed repetitions of the deep call: ms[0] (sparse: the scoring launches;
dense: query upload + GEMM), ms[1] (deep_select_rows) and the host-inclusive wall time of the call (query normalisation,
uploads, kernels, download of the [nq][k] arrays), min and max reported. Beside every k = 1 000 row the existing route on
the same batch in the same process: msr_batch_search at k = 1 000 on a resident batch (score and merge ms of
msr_batch_kernel_ms) with search_csr's wall time, DenseIndex.search_keys at k = 1 000 (gemm_ms, upload not included, and
select + merge ms), and the ratio deep / staged of the selection times and of the wall times. The k = 1 000 outputs of
both routes are compared (equal_k1000).

One JSON line on stdout, appended to --out if given.

    python scripts/gpu_deep_probe.py [--reps 5] [--shapes coco5k_i2t,flickr30k_t2i] [--out profiles/deep_probe.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(values):
    return dict(min=round(min(values), 3), max=round(max(values), 3))


def timed(fn, reps, ms_of):
    """One warm-up, then `reps` calls: (a, b) = ms_of(result) and the wall time of each -> three spreads and the last result."""
    rows, res = [], None
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        res = fn()
        wall = (time.perf_counter() - t0) * 1e3
        if rep:
            rows.append((*ms_of(res), wall))
    return [spread([r[j] for r in rows]) for j in range(3)], res


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def sparse_shape(m, wl, ks, reps, staged):
    qp, qt, qw = wl.queries
    rec = dict(n_docs=len(wl.docs[0]) - 1, nq=len(qp) - 1)
    with tempfile.TemporaryDirectory(prefix="msr_deep_") as tmp:
        path = m.build_index_from_csr(os.path.join(tmp, "d.idx"), *wl.docs, wl.n_terms)
        with m.SparseIndex(path, device=0) as ix:
            rec.update(tile_docs=ix.tile_docs, n_tiles=ix.n_tiles)
            for k in ks:
                (a, b, w), deep = timed(lambda: ix.search_deep(qp, qt, qw, k, with_ms=True), reps, lambda r: r[4])
                row = rec[f"deep_k{k}"] = dict(score_ms=a, deep_select_ms=b, host_inclusive_ms=w,
                                               mean_hits=round(float(deep[3].mean()), 1))
                note("sparse", rec["nq"], k, row)
                if k == 1000 and staged:
                    bt = ix.batch(qp, qt, qw, k)
                    try:
                        def run():
                            bt.search(k)
                            bt.sync()
                            return bt.kernel_ms()
                        (s, g, _), _ = timed(run, reps, lambda r: r)
                    finally:
                        bt.close()
                    (_, _, w2), usual = timed(lambda: ix.search_csr(qp, qt, qw, k), reps, lambda r: (0.0, 0.0))
                    rec["staged_k1000"] = dict(score_ms=s, merge_ms=g, host_inclusive_ms=w2)
                    rec["equal_k1000"] = bool(all((x == y).all() for x, y in zip(deep[:4], usual)))
                    rec["deep_over_staged_k1000"] = dict(
                        kernels=round((a["min"] + b["min"]) / (s["min"] + g["min"]), 3),
                        host_inclusive=round(w["min"] / w2["min"], 3))
                    note("sparse staged", rec["staged_k1000"], rec["deep_over_staged_k1000"], rec["equal_k1000"])
                del deep
    return rec


def dense_shape(precision, n, nq, h, ks, reps):
    from mllm_sparse_retrieval_amd.dense import DenseIndex

    rng = np.random.default_rng(1)
    p = rng.standard_normal((n, h), dtype=np.float32)
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    q = rng.standard_normal((nq, h), dtype=np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    rec = dict(rows=n, nq=nq, h=h, precision=precision)
    dix = DenseIndex(p, device=0, precision=precision)
    try:
        for k in ks:
            (a, b, w), deep = timed(lambda: dix.search_keys_deep(q, k), reps, lambda r: dix.last_ms)
            row = rec[f"deep_k{k}"] = dict(upload_gemm_ms=a, deep_select_ms=b, host_inclusive_ms=w)
            note("dense", precision, k, row)
            if k == 1000:
                (g, s, w2), usual = timed(lambda: dix.search_keys(q, k), reps, lambda r: dix.last_ms)
                rec["staged_k1000"] = dict(gemm_ms=g, select_merge_ms=s, host_inclusive_ms=w2)
                rec["equal_k1000"] = bool(all((x == y).all() for x, y in zip(deep, usual)))
                rec["deep_over_staged_k1000"] = dict(selection=round(b["min"] / s["min"], 3),
                                                     host_inclusive=round(w["min"] / w2["min"], 3))
                note("dense staged", rec["staged_k1000"], rec["deep_over_staged_k1000"], rec["equal_k1000"])
    finally:
        dix.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="coco5k_i2t,flickr30k_t2i")
    ap.add_argument("--commit", default="", help="label of the commit the figures are taken on")
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    a = ap.parse_args()
    import mllm_sparse_retrieval_amd as m
    from mllm_sparse_retrieval_amd import workloads

    rec = dict(probe="deep_lists", commit=a.commit, reps=a.reps)
    for name in a.shapes.split(","):
        if name == "coco5k_i2t":
            ks = (1000, 2000, 16384)
            rec[name] = dict(sparse=sparse_shape(m, workloads.coco5k("i2t"), ks, a.reps, True),
                             dense_f32=dense_shape("f32", 25010, 5000, 4096, ks, a.reps),
                             dense_fp16=dense_shape("fp16", 25010, 5000, 4096, ks, a.reps))
        elif name == "flickr30k_t2i":
            rec[name] = dict(sparse=sparse_shape(m, workloads.flickr30k_t2i(), (2000,), a.reps, False))
        else:
            sys.exit(f"unknown shape {name}")
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    bad = [n for n, r in rec.items() if isinstance(r, dict) for v in r.values() if v.get("equal_k1000") is False]
    if bad:
        sys.exit(f"deep and staged lists differ at k = 1000: {bad}")


if __name__ == "__main__":
    main()
