"""What a filtered search costs (msr_search_filtered, msr_dense_search_filtered) next to the unfiltered search of the same
batch in the same process (GPU).

Shape: the reference's hybrid shape, 25 010 docs x 5 000 queries at depth 1 000 (sparse: 120-term image queries, 4 tiles
of 8 192 docs; dense: H 4096, f32 and fp16). Doc sets:
  full      one set that holds every doc: the filter's own cost (mask pass, bitmap reads, the call's own host path);
  folds     the COCO 1K-fold protocol: five folds, doc o in fold (o * 5) // n_docs (a fold's docs are consecutive ids, so
            consecutive ordinals: whole tiles lie outside a fold and take the early exit), query i searches fold
            (i * 5) // nq;
  folds_mod the same five sizes spread over the index, doc o in fold o % 5: no tile is empty for any fold.
Per (route, sets): one warm-up and --reps timed repetitions; ms[0] / ms[1] of the filtered call (sparse: scoring launches
incl. the stage-1 merge / final merge; dense: query upload + GEMM / selection + merge) and the host-inclusive wall time,
min and max. Beside them the unfiltered search at k = 1 000: msr_batch_search on a resident batch (msr_batch_kernel_ms)
and search_csr's wall time; DenseIndex.search_keys (gemm_ms without the upload, select + merge ms). The full-set lists
are compared with the unfiltered ones (equal_full); the fold lists are checked for membership.

One JSON line on stdout, appended to --out if given.

    python scripts/gpu_filter_probe.py [--reps 5] [--out profiles/filter_probe.json]
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

K = 1000


def spread(values):
    return dict(min=round(min(values), 3), max=round(max(values), 3))


def timed(fn, reps, ms_of):
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


def doc_sets(n, nq):
    from mllm_sparse_retrieval_amd.filters import pack_doc_sets

    o, i = np.arange(n), np.arange(nq)
    q_fold = ((i * 5) // nq).astype(np.int32)
    return dict(full=(pack_doc_sets(np.ones((1, n), bool)), None, None),
                folds=(pack_doc_sets((o * 5) // n == np.arange(5)[:, None]), q_fold, (o * 5) // n),
                folds_mod=(pack_doc_sets(o % 5 == np.arange(5)[:, None]), q_fold, o % 5))


def members_only(idx, cnt, q_fold, fold_of):
    valid = np.arange(idx.shape[1])[None, :] < cnt[:, None]
    return bool((fold_of[np.where(valid, idx, 0)] == q_fold[:, None])[valid].all())


def sparse_route(m, wl, reps):
    qp, qt, qw = wl.queries
    n, nq = len(wl.docs[0]) - 1, len(qp) - 1
    rec = dict(n_docs=n, nq=nq, k=K)
    with tempfile.TemporaryDirectory(prefix="msr_filter_") as tmp:
        path = m.build_index_from_csr(os.path.join(tmp, "d.idx"), *wl.docs, wl.n_terms)
        with m.SparseIndex(path, device=0) as ix:
            rec.update(tile_docs=ix.tile_docs, n_tiles=ix.n_tiles)
            bt = ix.batch(qp, qt, qw, K)
            try:
                def run():
                    bt.search(K)
                    bt.sync()
                    return bt.kernel_ms()
                (s, g, _), _ = timed(run, reps, lambda r: r)
            finally:
                bt.close()
            (_, _, w), plain = timed(lambda: ix.search_csr(qp, qt, qw, K), reps, lambda r: (0.0, 0.0))
            rec["unfiltered"] = dict(score_ms=s, merge_ms=g, host_inclusive_ms=w)
            note("sparse unfiltered", rec["unfiltered"])
            for name, (bits, q_set, fold_of) in doc_sets(n, nq).items():
                (a, b, w), got = timed(lambda: ix.search_filtered(qp, qt, qw, K, bits, q_set, with_ms=True), reps, lambda r: r[4])
                row = rec[name] = dict(score_ms=a, merge_ms=b, host_inclusive_ms=w, mean_hits=round(float(got[3].mean()), 1))
                if name == "full":
                    row["equal_full"] = bool(all((x == y).all() for x, y in zip(got[:4], plain)))
                else:
                    row["members_only"] = members_only(got[0], got[3], q_set, fold_of)
                note("sparse", name, row)
    return rec


def dense_route(precision, n, nq, h, reps):
    from mllm_sparse_retrieval_amd.dense import DenseIndex

    rng = np.random.default_rng(1)
    p = rng.standard_normal((n, h), dtype=np.float32)
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    q = rng.standard_normal((nq, h), dtype=np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    rec = dict(rows=n, nq=nq, h=h, k=K, precision=precision)
    dix = DenseIndex(p, device=0, precision=precision)
    try:
        (g, s, w), plain = timed(lambda: dix.search_keys(q, K), reps, lambda r: dix.last_ms)
        rec["unfiltered"] = dict(gemm_ms=g, select_merge_ms=s, host_inclusive_ms=w)
        note("dense", precision, "unfiltered", rec["unfiltered"])
        for name, (bits, q_set, fold_of) in doc_sets(n, nq).items():
            (a, b, w), got = timed(lambda: dix.search_keys_filtered(q, K, bits, q_set), reps, lambda r: dix.last_ms)
            row = rec[name] = dict(upload_gemm_ms=a, select_merge_ms=b, host_inclusive_ms=w)
            if name == "full":
                row["equal_full"] = bool(all((x == y).all() for x, y in zip(got, plain)))
            else:
                row["members_only"] = members_only(got[0], got[2], q_set, fold_of)
            note("dense", precision, name, row)
    finally:
        dix.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--commit", default="", help="label of the commit the figures are taken on")
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    a = ap.parse_args()
    import mllm_sparse_retrieval_amd as m
    from mllm_sparse_retrieval_amd import workloads

    rec = dict(probe="filtered_search", commit=a.commit, reps=a.reps, shape="coco5k_i2t")
    rec["sparse"] = sparse_route(m, workloads.coco5k("i2t"), a.reps)
    rec["dense_f32"] = dense_route("f32", 25010, 5000, 4096, a.reps)
    rec["dense_fp16"] = dense_route("fp16", 25010, 5000, 4096, a.reps)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    bad = [r for r in ("sparse", "dense_f32", "dense_fp16") for v in rec[r].values()
           if isinstance(v, dict) and (v.get("equal_full") is False or v.get("members_only") is False)]
    if bad:
        sys.exit(f"filtered lists are wrong: {bad}")


if __name__ == "__main__":
    main()
