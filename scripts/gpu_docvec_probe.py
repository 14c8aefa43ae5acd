"""What reading doc vectors out of the index costs (msr_doc_vectors), next to its floor (GPU).

The Flickr30K-shape workload (31 014 docs). One warm-up and --reps timed repetitions of
  - the whole-index export: every doc in one call, ms = HIP-event times of {count pass, fill pass, ordering pass} and the
    host-inclusive wall time of the filling call;
  - a 64-doc call (ordinals spread evenly over the index), the same figures.
Beside them the floor they are to be read against: the count pass and the fill pass each stream the postings of every
tile that holds a listed doc once, so two reads of the handle's resident_bytes at the bandwidth msr_device_copy_gbs
reports in the same run. Every repetition kept, and the export checked against the CSR the index was built from on the
last repetition.

One JSON line on stdout, appended to --out if given.

    python scripts/gpu_docvec_probe.py [--reps 5] [--out FILE]
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
    return dict(min=round(min(values), 4), max=round(max(values), 4), all=[round(v, 4) for v in values])


def timed(ix, ords, reps):
    ms, wall = [], []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        out = ix.doc_vectors(ords, with_ms=True)
        dt = (time.perf_counter() - t0) * 1e3
        if rep:  # (the first repetition warms up)
            ms.append(out[3])
            wall.append(dt)
    rec = {name: spread([x[i] for x in ms]) for i, name in enumerate(("count_ms", "fill_ms", "order_ms"))}
    rec["host_inclusive_ms"] = spread(wall)  # (the sizing call and the filling call)
    return rec, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import mllm_sparse_retrieval_amd as m
    from mllm_sparse_retrieval_amd import workloads

    wl = workloads.flickr30k_t2i()
    dp, dt, dw = wl.docs
    n_docs = len(dp) - 1
    rec = dict(probe="doc_vectors", n_docs=n_docs, n_terms=wl.n_terms, reps=a.reps)
    with tempfile.TemporaryDirectory(prefix="msr_docvec_") as tmp:
        ids = ["%07d" % i for i in range(n_docs)]  # ordinal == input row
        path = m.build_index_from_csr(os.path.join(tmp, "x.idx"), dp, dt, dw, wl.n_terms, doc_ids=ids)
        with m.SparseIndex(path, device=0) as ix:
            gbs = m.index.device_copy_gbs(0)
            rec.update(tile_docs=ix.tile_docs, n_tiles=ix.n_tiles, n_postings=ix.n_postings, n_dense=ix.n_dense,
                       resident_bytes=ix.resident_bytes, copy_gbs=round(gbs, 1),
                       floor_two_reads_ms=round(2 * ix.resident_bytes / (gbs * 1e9) * 1e3, 4))
            rec["whole_index"], (ptr, term, w, _) = timed(ix, np.arange(n_docs, dtype=np.uint32), a.reps)
            order = np.lexsort((np.asarray(dt), np.repeat(np.arange(n_docs), np.diff(np.asarray(dp, np.int64)))))
            rec["whole_index"]["entries"] = int(ptr[-1])
            rec["whole_index"]["equals_input_csr"] = bool(
                (ptr == np.asarray(dp, np.int64)).all() and (term == np.asarray(dt)[order]).all()
                and (w == np.asarray(dw)[order]).all())
            few = np.linspace(0, n_docs - 1, 64).astype(np.uint32)
            rec["docs_64"], (ptr, _, _, _) = timed(ix, few, a.reps)
            rec["docs_64"]["entries"] = int(ptr[-1])
            rec["docs_64"]["tiles_touched"] = len({int(o) // ix.tile_docs for o in few})
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
