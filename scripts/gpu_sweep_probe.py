"""What an alpha sweep costs as ONE msr_hybrid_sweep call next to eleven msr_hybrid_search[_f32] calls (GPU).

The reference's own hybrid run, i2t: 5 000 image queries x 25 010 caption docs, H = 4096, depth 1000, 8192-doc tiles,
--remove_query; alphas 0, 0.1, ..., 1. Per precision (fp16 and f32 handles) and per k (200 and 1000), one warm-up and
--reps timed repetitions each of
  (i)  one dense.hybrid_sweep call: the library's device-event ms per slot {sparse = candidate kernel, dense_gemm, fusion
       = the union pass's fusion kernel, sweep = the sweep kernels summed, groups} and host-inclusive wall ms;
  (ii) eleven dense.hybrid_search / hybrid_search_f32 calls, one per alpha, in the same session: the ms slots summed over
       the eleven calls, the `fusion` slot of ONE call, and the host-inclusive wall ms of the eleven together. This code
       is the parent commit's, so (ii) is the parent's cost of the sweep.
min / max over the repetitions of every figure, `sweep_ms_per_alpha` = sweep / 11 next to `plain_fusion_ms_per_call`, and
`identical`: whether the eleven slices of (i) equal the eleven results of (ii) bit for bit (ordinals, score bits, counts).

Each precision runs in a child process of its own under a time limit (--step, --limit seconds); a child that fails or
runs out of time ends the probe: nothing else is started on the GPU after it. One JSON line on stdout, appended to --out
if given.

    python scripts/gpu_sweep_probe.py [--reps 5] [--commit LABEL] [--out profiles/sweep_probe.json]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, DEPTH, N_TERMS, N, NQ, TILE = 4096, 1000, 30000, 25010, 5000, 8192
ALPHAS = [round(0.1 * i, 1) for i in range(11)]
KS = (200, 1000)
SLOTS = ("sparse", "dense_gemm", "fusion", "sweep")


def spread(rows):
    """[{name: value}] per repetition -> {name: {min, max}}"""
    return {a: dict(min=round(min(r[a] for r in rows), 3), max=round(max(r[a] for r in rows), 3)) for a in rows[0]}


def step(prec, reps):
    sys.path.insert(0, ROOT)
    import mllm_sparse_retrieval_amd as m
    from mllm_sparse_retrieval_amd import dense, workloads

    docs, (qp, qt, qw), p, q = workloads.hybrid_vectors(N, NQ, H, N_TERMS)
    topk = dense.hybrid_search_f32 if prec == "f32" else dense.hybrid_search
    rec = {}
    with tempfile.TemporaryDirectory(prefix="msr_sw_") as tmp:
        path = m.build_index_from_csr(os.path.join(tmp, "h.idx"), *docs, N_TERMS, tile_docs=TILE)
        with m.SparseIndex(path, device=0) as ix:
            r2o = dense.row_to_ordinal(ix, [str(i) for i in range(N)])
            self_ord = r2o[:NQ].astype(np.int32)
            dix = dense.DenseIndex(p, device=0, precision=prec)
            try:
                for k in KS:
                    sweep = lambda: dense.hybrid_sweep(ix, dix, qp, qt, qw, q, DEPTH, k, ALPHAS, r2o, self_ord)  # noqa: E731
                    plain = lambda: [topk(ix, dix, qp, qt, qw, q, DEPTH, k, a, r2o, self_ord) for a in ALPHAS]  # noqa: E731
                    sweep(), plain()  # warm-up: ordinal rows, scratch, first launches
                    s_rows, p_rows, s_out, p_out = [], [], None, None
                    for _ in range(reps):
                        t0 = time.perf_counter()
                        s_out = sweep()
                        wall = (time.perf_counter() - t0) * 1e3
                        s_rows.append(dict({a: s_out[3][a] for a in SLOTS}, host_inclusive_ms=wall,
                                           sweep_ms_per_alpha=s_out[3]["sweep"] / len(ALPHAS)))
                        groups = s_out[3]["groups"]
                        t0 = time.perf_counter()
                        p_out = plain()
                        wall = (time.perf_counter() - t0) * 1e3
                        row = {a: sum(o[3][a] for o in p_out) for a in SLOTS[:3]}
                        p_rows.append(dict(row, host_inclusive_ms=wall, plain_fusion_ms_per_call=row["fusion"] / len(ALPHAS),
                                           plain_kernels_ms_per_call=sum(row.values()) / len(ALPHAS)))
                    same = all((s_out[0][a] == o[0]).all() and (s_out[1][a].view(np.uint32) == o[1].view(np.uint32)).all() and
                               (s_out[2][a] == o[2]).all() for a, o in enumerate(p_out))
                    rec[f"k{k}"] = dict(sweep_call=spread(s_rows), eleven_plain_calls=spread(p_rows), groups=groups,
                                        identical=bool(same), members_mean=float(s_out[2].mean()))
            finally:
                dix.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=420, help="seconds one precision's child process may take")
    ap.add_argument("--commit", default="", help="label of the commit the figures are taken on")
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    ap.add_argument("--step", default=None, choices=["fp16", "f32"], help="(internal) run one precision in this process")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step(a.step, a.reps)))
        return 0
    rec = dict(probe="sweep", commit=a.commit, n=N, nq=NQ, h=H, depth=DEPTH, tile_docs=TILE, alphas=ALPHAS, reps=a.reps,
               remove_query=True)
    for prec in ("fp16", "f32"):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--step", prec, "--reps", str(a.reps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:  # a fault, an abort or the time limit: nothing more is started on the GPU
            rec[prec] = dict(failed=r.returncode)
            print(json.dumps(rec))
            return 1
        rec[prec] = json.loads(r.stdout.strip().splitlines()[-1])
        print(f"{prec}: done", file=sys.stderr, flush=True)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
