"""What filtered deep hybrid search costs (msr_hybrid_deep_filtered, dense.hybrid_deep_filtered) on the reference's hybrid
shape (GPU): 25 010 docs x 5 000 queries, H 4096, fp16 and f32 handles, remove_query on, depth 1 000.

Per handle, with one alpha (k = 2 000, both depth lists, sources and extremes) and with eleven (k = 1 000, no lists), warm,
--reps repetitions, min - max. The baseline is msr_hybrid_deep on the same handles in the same process, ALTERNATING with the
new call lap by lap (baseline, run i, baseline, run ii, ...), so both see the same clocks:
  baseline   msr_hybrid_deep: the parent commit's code path. Its laps are split in two halves (first_half / second_half): the
             distance between the halves is the spread that repeated baseline runs have among themselves.
  i          every query q_set = -1 (no pass holds a filtered query: the launches are the baseline's);
  ii         one full set for every query (the filtered dump and mask_key_rows run, nothing is masked away);
  iii        five fold sets, doc o in fold o mod 5 (members interleaved over the tiles, as COCO doc ids are), query i in
             fold i mod 5.
Per lap the seven ms slots {sparse scoring (the filtered dump), query upload + GEMM, the two depth selections, fuse_rows
summed, fused selections summed, passes, mask_key_rows summed} and the host-inclusive wall time. For mask_key_rows: the
bytes it moves (8 per column of a filtered row: a 4-byte key read and written) over its time, next to msr_device_copy_gbs
from the same process. Runs i and ii are checked bit for bit against the baseline's outputs; run iii's docs against the sets.

One JSON line on stdout, appended to --out if given.

    python scripts/gpu_hybrid_filtered_probe.py [--reps 5] [--precisions fp16,f32] [--out profiles/hybrid_filtered_probe.json]
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
H, ALPHA, N_TERMS, N, NQ, DEPTH, FOLDS = 4096, 0.3, 30000, 25010, 5000, 1000, 5
A11 = [round(0.1 * i, 1) for i in range(11)]
SLOTS = ("sparse", "dense_gemm", "depth_select", "fuse_rows", "fused_select", "mask")


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def spread(values):
    return dict(min=round(min(values), 3), max=round(max(values), 3))


def summary(laps, walls):
    out = {s: spread([l.get(s, 0.0) for l in laps]) for s in SLOTS}
    out["passes"] = int(laps[0]["passes"])
    out["kernels_ms_min"] = round(min(sum(l.get(s, 0.0) for s in SLOTS) for l in laps), 3)
    out["host_inclusive_ms"] = spread(walls)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--precisions", default="fp16,f32")
    ap.add_argument("--commit", default="", help="label of the commit the figures are taken on")
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    a = ap.parse_args()
    import mllm_sparse_retrieval_amd as m
    from mllm_sparse_retrieval_amd import dense, workloads
    from mllm_sparse_retrieval_amd.filters import pack_doc_sets

    docs, (qp, qt, qw), p, q = workloads.hybrid_vectors(N, NQ, H, N_TERMS)
    rec = dict(probe="hybrid_filtered", commit=a.commit, reps=a.reps, n=N, nq=NQ, h=H, alpha=ALPHA, depth=DEPTH, remove_query=True,
               device_copy_gbs=round(m.device_copy_gbs(0), 1))
    bad = []
    o = np.arange(N)
    full = pack_doc_sets(np.ones((1, N), bool))
    folds = pack_doc_sets(np.stack([o % FOLDS == f for f in range(FOLDS)]))
    fold_q = (np.arange(NQ) % FOLDS).astype(np.int32)
    runs = (("i_unfiltered", full, np.full(NQ, -1, np.int32), 0), ("ii_full_set", full, np.zeros(NQ, np.int32), NQ),
            ("iii_five_folds", folds, fold_q, NQ))
    with tempfile.TemporaryDirectory(prefix="msr_hf_") as tmp:
        path = m.build_index_from_csr(os.path.join(tmp, "h.idx"), *docs, N_TERMS)
        with m.SparseIndex(path, device=0) as ix:
            r2o = dense.row_to_ordinal(ix, [str(i) for i in range(N)])
            self_ord = r2o[:NQ].astype(np.int32)
            rec.update(tile_docs=ix.tile_docs, n_tiles=ix.n_tiles)
            ld_d = (N + 255) // 256 * 256
            for prec in a.precisions.split(","):
                dix = dense.DenseIndex(p, device=0, precision=prec)
                r = rec[prec] = {}
                try:
                    for tag, alphas, k, lists in (("one_alpha", [ALPHA], 2 * DEPTH, True), ("eleven_alphas", A11, 1000, False)):
                        def base():
                            return dense.hybrid_deep(ix, dix, qp, qt, qw, q, DEPTH, k, alphas, r2o, self_ord, with_lists=lists)

                        def filt(bits, q_set):
                            return dense.hybrid_deep_filtered(ix, dix, qp, qt, qw, q, DEPTH, k, alphas, r2o, bits, q_set, self_ord,
                                                              with_lists=lists)

                        laps = {name: [] for name in ("baseline",) + tuple(x[0] for x in runs)}
                        walls = {name: [] for name in laps}
                        last = {}
                        for rep in range(a.reps + 1):                  # (lap 0 warms every route up)
                            for name, bits, q_set, _ in runs:
                                for who, fn in (("baseline", base), (name, lambda: filt(bits, q_set))):
                                    t0 = time.perf_counter()
                                    res = fn()
                                    wall = (time.perf_counter() - t0) * 1e3
                                    if rep:
                                        laps[who].append(res.ms)
                                        walls[who].append(wall)
                                    last[who] = res
                        row = r[tag] = dict(k=k)
                        nb = len(laps["baseline"])
                        row["baseline"] = summary(laps["baseline"], walls["baseline"])
                        row["baseline"]["first_half"] = summary(laps["baseline"][:nb // 2], walls["baseline"][:nb // 2])
                        row["baseline"]["second_half"] = summary(laps["baseline"][nb // 2:], walls["baseline"][nb // 2:])
                        for name, bits, q_set, n_filtered in runs:
                            s = row[name] = summary(laps[name], walls[name])
                            s["kernels_over_baseline"] = round(s["kernels_ms_min"] / row["baseline"]["kernels_ms_min"], 4)
                            if n_filtered:
                                moved = 8 * ld_d * n_filtered
                                s["mask_key_rows_bytes"] = moved
                                s["mask_key_rows_gbs"] = round(moved / (s["mask"]["min"] * 1e-3) / 1e9, 1)
                            res, ref = last[name], last["baseline"]
                            if name != "iii_five_folds":
                                same = bool((res.ords == ref.ords).all() and (res.n == ref.n).all() and (res.members == ref.members).all()
                                            and (res.scores.view(np.uint32) == ref.scores.view(np.uint32)).all())
                                s["bit_equal_to_baseline"] = same
                                if not same:
                                    bad.append(f"{prec} {tag} {name}: differs from msr_hybrid_deep")
                            else:
                                live = res.ords[0] != 0xFFFFFFFF
                                in_set = bool(((res.ords[0] % FOLDS == fold_q[:, None]) | ~live).all())
                                s["every_doc_in_its_fold"] = in_set
                                s["mean_members"] = round(float(res.members.mean()), 1)
                                if not in_set:
                                    bad.append(f"{prec} {tag}: a doc outside its query's fold")
                            note(prec, tag, name, s)
                        note(prec, tag, "baseline", row["baseline"])
                finally:
                    dix.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    if bad:
        sys.exit("; ".join(bad))


if __name__ == "__main__":
    main()
