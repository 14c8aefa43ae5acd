"""What explaining hits costs (msr_explain_docs) next to the nearest existing kernel (GPU).

The Flickr30K-shape workload (31 014 docs, caption queries of 8-15 terms), its first --queries queries, each with its
top-10 hits (msr_search_csr) as listed docs. One warm-up and --reps timed repetitions of
  - msr_explain_docs: ms (zeroing the output + the explain launch) and the host-inclusive wall time of the call;
  - msr_rank_docs on the same targets: ms[0], the gather launch — it walks the same segments, through the accumulation.
Every repetition kept, min and max reported, and the identity sum(q_w * d_w) == score checked on the last repetition.

One JSON line on stdout, appended to --out if given.

    python scripts/gpu_explain_probe.py [--reps 5] [--queries 10000] [--out FILE]
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


def spread(values):
    return dict(min=round(min(values), 3), max=round(max(values), 3), all=[round(v, 3) for v in values])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import mllm_sparse_retrieval_amd as m
    from mllm_sparse_retrieval_amd import workloads

    wl = workloads.flickr30k_t2i()
    qp, qt, qw = wl.queries
    nq = min(a.queries, len(qp) - 1)
    qp = np.asarray(qp[:nq + 1], dtype=np.int64)
    qt, qw = np.asarray(qt[:qp[-1]], dtype=np.int32), np.asarray(qw[:qp[-1]], dtype=np.int32)
    rec = dict(probe="explain_docs", n_docs=len(wl.docs[0]) - 1, nq=nq, reps=a.reps, entries=int(qp[-1]))
    with tempfile.TemporaryDirectory(prefix="msr_explain_") as tmp:
        path = m.build_index_from_csr(os.path.join(tmp, "x.idx"), *wl.docs, wl.n_terms)
        with m.SparseIndex(path, device=0) as ix:
            ords, _, u32, n = ix.search_csr(qp, qt, qw, 10)
            t_ptr = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
            t_ord = np.concatenate([ords[i, :n[i]] for i in range(nq)]).astype(np.uint32)
            pairs = len({(i, int(o) // ix.tile_docs) for i in range(nq) for o in ords[i, :n[i]]})
            rec.update(tile_docs=ix.tile_docs, n_tiles=ix.n_tiles, targets=len(t_ord), pairs=pairs)
            ex, ex_wall, gather = [], [], []
            for rep in range(a.reps + 1):
                t0 = time.perf_counter()
                x_ptr, doc_w, ms = ix.explain_docs(qp, qt, qw, t_ptr, t_ord, with_ms=True)
                dt = (time.perf_counter() - t0) * 1e3
                _, scores, rms = ix.rank_docs(qp, qt, qw, t_ptr, t_ord, with_ms=True)
                if rep:  # (the first repetition warms up)
                    ex.append(ms)
                    ex_wall.append(dt)
                    gather.append(rms[0])
            rec.update(slots=int(x_ptr[-1]), matched=int(np.count_nonzero(doc_w)))
            w_rep = np.maximum(qw, 0).astype(np.int64)
            got = np.zeros(len(t_ord), dtype=np.int64)
            e = 0
            for i in range(nq):
                w = w_rep[qp[i]:qp[i + 1]]
                for _ in range(int(n[i])):
                    got[e] = int(w @ doc_w[x_ptr[e]:x_ptr[e + 1]].astype(np.int64))
                    e += 1
            want = np.concatenate([u32[i, :n[i]] for i in range(nq)]).astype(np.int64)
            rec["identity_holds"] = bool((got == want).all() and (got == scores.astype(np.int64)).all())
            rec["explain_ms"] = spread(ex)
            rec["explain_host_inclusive_ms"] = spread(ex_wall)
            rec["rank_gather_ms"] = spread(gather)
            rec["explain_over_gather_min"] = round(min(ex) / min(gather), 3)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
