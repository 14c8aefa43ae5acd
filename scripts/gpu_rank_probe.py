"""What exact ranks cost (msr_rank_docs) next to the top-10 search of the same batch (GPU).

Two shapes, each with every query's judged docs as targets:
  flickr30k_t2i   the headline batch: 31 014 docs, 155 070 caption queries (8-15 terms: the light accumulation), one
                  target each (the caption's image);
  coco5k_i2t      the C3 i->t shape: 25 010 caption docs, 5 000 image queries (120 terms: the general accumulation),
                  five targets each (the image's captions).
Per shape, one warm-up and --reps timed repetitions of
  - msr_batch_search at k = 10 on a resident batch: HIP-event ms of the scoring launches and of the merge
    (msr_batch_kernel_ms). This is the figure to take on the parent commit too: --search_only measures nothing else, and
    --tree ROOT imports the package (and its libmsr.so) from another checkout;
  - msr_rank_docs: ms[0] (gather launch), ms[1] (count launches + reduction) and the host-inclusive wall time of the call
    (query normalisation, pair list, uploads, kernels, download),
every repetition kept, min and max reported. Also recorded: the (query, tile) pairs the gather phase accumulates as a
share of all pairs, and the metrics of the ranks (ranks.rank_metrics) as a plausibility check.

One JSON line on stdout, appended to --out if given. Kernel times without the events: run under
rocprofv3 --kernel-trace --stats.

    python scripts/gpu_rank_probe.py [--reps 5] [--commit LABEL] [--out profiles/rank_probe.json]
    python scripts/gpu_rank_probe.py --search_only --tree PARENT_CHECKOUT --commit parent [--out ...]
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


def shape(m, wl, targets_of, reps, search_only):
    qp, qt, qw = wl.queries
    nq = len(qp) - 1
    rec = dict(n_docs=len(wl.docs[0]) - 1, nq=nq, reps=reps)
    with tempfile.TemporaryDirectory(prefix="msr_rank_") as tmp:
        path = m.build_index_from_csr(os.path.join(tmp, "r.idx"), *wl.docs, wl.n_terms)
        with m.SparseIndex(path, device=0) as ix:
            rec.update(tile_docs=ix.tile_docs, n_tiles=ix.n_tiles)
            b = ix.batch(qp, qt, qw, 10)
            try:
                score, merge = [], []
                for rep in range(reps + 1):
                    b.search(10)
                    b.sync()
                    if rep:  # (the first repetition warms up)
                        s, g = b.kernel_ms()
                        score.append(s)
                        merge.append(g)
                rec["search_k10"] = dict(score_ms=spread(score), merge_ms=spread(merge),
                                         score_plus_merge_ms=spread([s + g for s, g in zip(score, merge)]))
            finally:
                b.close()
            if search_only or not hasattr(ix, "rank_docs"):
                return rec
            from mllm_sparse_retrieval_amd.ranks import rank_metrics

            ord_of = {d: o for o, d in enumerate(ix.docid_table().tolist())}
            lists = [[ord_of[str(d)] for d in targets_of(i)] for i in range(nq)]
            t_ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
            t_ord = np.asarray([o for x in lists for o in x], dtype=np.uint32)
            pairs = len({(i, o // ix.tile_docs) for i, x in enumerate(lists) for o in x})
            rec.update(targets=len(t_ord), gather_pairs=pairs, all_pairs=nq * ix.n_tiles,
                       gather_pair_share=round(pairs / (nq * ix.n_tiles), 4))
            gather, count, wall, ranks = [], [], [], None
            for rep in range(reps + 1):
                t0 = time.perf_counter()
                ranks, _, ms = ix.rank_docs(qp, qt, qw, t_ptr, t_ord, with_ms=True)
                dt = (time.perf_counter() - t0) * 1e3
                if rep:
                    gather.append(ms[0])
                    count.append(ms[1])
                    wall.append(dt)
            rec["rank_docs"] = dict(gather_ms=spread(gather), count_reduce_ms=spread(count), host_inclusive_ms=spread(wall))
            rec["count_over_search_score_min"] = round(min(count) / min(score), 3)
            met = rank_metrics(ranks, t_ptr, ix.n_docs)
            rec["metrics"] = dict(recall={str(k): round(v, 5) for k, v in met["recall"].items()}, mrr=round(met["mrr"], 5),
                                  medr=met["medr"], meanr=round(met["meanr"], 2), n_unranked=met["n_unranked"],
                                  max_rank=int(ranks.max()))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--search_only", action="store_true", help="only the k = 10 search (what the parent commit can run)")
    ap.add_argument("--tree", default=ROOT, help="repository root whose package (and libmsr.so) is measured")
    ap.add_argument("--shapes", default="flickr30k_t2i,coco5k_i2t")
    ap.add_argument("--commit", default="", help="label of the commit the figures are taken on")
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import mllm_sparse_retrieval_amd as m
    from mllm_sparse_retrieval_amd import workloads

    rec = dict(probe="rank_docs", commit=a.commit, search_only=bool(a.search_only))
    for name in a.shapes.split(","):
        if name == "flickr30k_t2i":
            rec[name] = shape(m, workloads.flickr30k_t2i(), lambda i: [i // 5], a.reps, a.search_only)
        elif name == "coco5k_i2t":
            rec[name] = shape(m, workloads.coco5k("i2t"), lambda i: range(5 * i, 5 * i + 5), a.reps, a.search_only)
        else:
            sys.exit(f"unknown shape {name}")
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
