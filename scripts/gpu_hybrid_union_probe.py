"""What the whole fused union costs (msr_hybrid_search_union) next to the top-k hybrid calls, and the CLI gate (GPU).

kernels (default): the reference's own hybrid run, i2t: 5 000 image queries x 25 010 caption docs, H = 4096, depth 1000,
alpha 0.5, --remove_query, fp16 and f32. Per precision, one warm-up and --reps timed calls each of
  - hybrid_search / hybrid_search_f32 at k = 1000 (the call that exists without the union; run this script on the parent
    commit too: a tree without hybrid_search_union measures only this part),
  - hybrid_search_union with all arrays and with with_lists=False,
the library's device-event ms {sparse = candidate kernel, dense_gemm, fusion} of EVERY repetition (so the spread is in
the record), host-inclusive wall ms, and the host time of fusion.union_to_runs over the full result.

--gate ENC: wall time of `search` through the CLI, each run a fresh process, from process start to exit (the three
.trec files are written before the process ends), best of --reps, on the output of
    encode --synthetic coco --n_images 5000 --sparse_output_dir ENC/sparse --dense_output_dir ENC/dense --dense_dim D
    index --input ENC/sparse
with --query_type image --depth 1000 --remove_query, for the routes named by --routes: union (--fusion_union), host
(--host_fusion), default (neither). --tree names the repository root whose package runs the search (the parent commit's
checkout for the figures that are taken there), --commit labels the record.

One JSON line on stdout, appended to --out if given. Kernel times without the events: run under
rocprofv3 --kernel-trace --stats.

    python scripts/gpu_hybrid_union_probe.py [--reps 5] [--commit LABEL] [--out profiles/hybrid_union_probe.json]
    python scripts/gpu_hybrid_union_probe.py --gate ENC --routes union,host,default [--tree ROOT] [--reps 3] ...
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, DEPTH, ALPHA, N_TERMS, N, NQ = 4096, 1000, 0.5, 30000, 25010, 5000


def timed(fn, reps):
    fn()  # warm-up: ordinal rows, scratch, first launches
    walls, laps, out = [], [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        walls.append(round((time.perf_counter() - t0) * 1e3, 3))
        laps.append({a: round(b, 3) for a, b in out[-1].items() if a != "dense_select"})
    return out, dict(kernel_ms_all=laps, kernel_ms_min={a: min(l[a] for l in laps) for a in laps[0]},
                     kernel_ms_max={a: max(l[a] for l in laps) for a in laps[0]},
                     host_inclusive_ms=min(walls), host_inclusive_ms_all=walls)


def kernels(reps):
    sys.path.insert(0, ROOT)
    import mllm_sparse_retrieval_amd as m
    from mllm_sparse_retrieval_amd import dense, fusion, workloads

    union = getattr(dense, "hybrid_search_union", None)  # (absent on the parent commit)
    docs, (qp, qt, qw), p, q = workloads.hybrid_vectors(N, NQ, H, N_TERMS)
    rec = dict(n=N, nq=NQ, h=H, depth=DEPTH, alpha=ALPHA, remove_query=True, reps=reps)
    with tempfile.TemporaryDirectory(prefix="msr_hu_") as tmp:
        path = m.build_index_from_csr(os.path.join(tmp, "h.idx"), *docs, N_TERMS)
        with m.SparseIndex(path, device=0) as ix:
            r2o = dense.row_to_ordinal(ix, [str(i) for i in range(N)])
            self_ord = r2o[:NQ].astype(np.int32)
            table = ix.docid_table()
            for prec, topk in (("fp16", dense.hybrid_search), ("f32", dense.hybrid_search_f32)):
                dix = dense.DenseIndex(p, device=0, precision=prec)
                try:
                    r = {}
                    _, r["top1000"] = timed(lambda: topk(ix, dix, qp, qt, qw, q, DEPTH, 1000, ALPHA, r2o, self_ord), reps)
                    if union:
                        res, r["union_all_arrays"] = timed(
                            lambda: union(ix, dix, qp, qt, qw, q, DEPTH, ALPHA, r2o, self_ord), reps)
                        _, r["union_without_lists"] = timed(
                            lambda: union(ix, dix, qp, qt, qw, q, DEPTH, ALPHA, r2o, self_ord, with_lists=False), reps)
                        r["union_members_mean"] = float(res[2].mean())
                        r["fusion_kernel_ratio_union_over_top1000"] = round(
                            r["union_all_arrays"]["kernel_ms_min"]["fusion"] / r["top1000"]["kernel_ms_min"]["fusion"], 3)
                        t0 = time.perf_counter()
                        fusion.union_to_runs([str(i) for i in range(NQ)], table, res[0], res[2], res[1], *res[3:7])
                        r["union_to_runs_host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                    rec[prec] = r
                finally:
                    dix.close()
    return rec


def gate(enc, routes, tree, reps):
    flags = dict(union=["--fusion_union"], host=["--host_fusion"], default=[])
    rec = dict(reps=reps, routes={})  # (which tree ran: the record's `commit` label)
    import pickle

    with open(os.path.join(enc, "dense", "query.pkl"), "rb") as f:
        rec["dense_dim"] = int(np.asarray(pickle.load(f)[0]).shape[1])
    for route in routes:
        walls = []
        for _ in range(reps):
            out = tempfile.mkdtemp(prefix=f"msr_gate_{route}_")
            cmd = [sys.executable, "-m", "mllm_sparse_retrieval_amd", "search", "--sparse_index", os.path.join(enc, "sparse"),
                   "--passage_reps", os.path.join(enc, "dense"), "--query_type", "image", "--depth", "1000",
                   "--remove_query", "--quiet", "--save_dir", out, *flags[route]]
            t0 = time.perf_counter()
            subprocess.run(cmd, check=True, cwd=tree, timeout=1500)
            walls.append(round(time.perf_counter() - t0, 2))
            sizes = {n: os.path.getsize(os.path.join(out, n)) for n in ("sparse.trec", "dense.trec", "fusion.trec")}
            shutil.rmtree(out)
        rec["routes"][route] = dict(wall_s=min(walls), wall_s_all=walls, trec_bytes=sizes)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gate", default=None, help="directory with sparse/ and dense/ of one synthetic coco encode")
    ap.add_argument("--routes", default="union,host,default")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--commit", default="", help="label of the commit the figures are taken on")
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    a = ap.parse_args()
    rec = dict(probe="hybrid_union", commit=a.commit)
    if a.gate:
        rec["gate"] = gate(a.gate, a.routes.split(","), a.tree, a.reps)
    else:
        rec["kernels"] = kernels(a.reps)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
