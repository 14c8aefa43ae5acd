"""encode -> index -> search, with the reference's flag names (src/arguments.py:57-68, scripts/*.sh).

    python -m mllm_sparse_retrieval_amd encode --synthetic flickr --sparse_output_dir out/        (no MLLM here)
    python -m mllm_sparse_retrieval_amd index  --input out/ [--index out/index] --threads 16       (sparse_index.sh)
    python -m mllm_sparse_retrieval_amd search --sparse_index out/ --depth 10 --query_type text \\
           --dataset_name flickr --queries out/query.tsv --qrels out/qrels.csv --save_dir runs/   (search_sparse.sh)
           [--ranks: exact rank of every judged doc at any depth -> recall / MRR / MedR / MeanR, sparse.ranks.tsv]
           [--explain N: per-token query weight x doc weight of the first N hits and the judged docs, sparse.explain.tsv]
           [--alphas 0,0.1,...,1: hybrid on the GPU, ONE msr_hybrid_sweep call fuses the scoring at every alpha -> one recall line
            per alpha, fusion.sweep.tsv; --sweep_runs: fusion.alpha_{a}.trec per alpha]
           [--deep: --depth up to 16384 (msr_search_deep; dense-only: msr_dense_search_deep; hybrid: with --host_fusion)]
           [--fusion_deep: hybrid on the GPU at --depth up to 16384, ONE msr_hybrid_deep call -> sparse.trec, dense.trec and
            the whole fused union in fusion.trec; with --alphas the sweep outputs]
           [--fusion_filtered --doc_sets F --query_sets F: --fusion_deep among the docs of each query's set, ONE
            msr_hybrid_deep_filtered call, the same outputs]
    python -m mllm_sparse_retrieval_amd search --passage_reps dense/ --depth 10 --remove_query \\
           --qrels out/qrels.csv --save_dir runs/                                                  (search_dense.sh)
           [--ranks: exact rank of every judged row at any depth (msr_dense_rank_rows) -> the same metrics, dense.ranks.tsv]

    python -m mllm_sparse_retrieval_amd vectors --sparse_index out/ [--docids a,b,c | --docids_file F] [--output FILE]
           (the stored doc vectors back out of the index, jsonl in the encode format; no counterpart script)

    python -m mllm_sparse_retrieval_amd eval   --runs_dir runs/ --qrels out/qrels.csv --dataset_name flickr \
           --query_type text [--compat-denominator --world_size 4]                                (recall of TREC runs)

`encode` writes exactly the files src/encode.py:412-426 writes (corpus_{shard}.jsonl, query.tsv); `index` accepts and
ignores pyserini's --collection/--generator/--impact/--pretokenized; `search` prints recall in the reference's format
(src/metrices.py:103-137) and writes TREC runs (src/hybrid.py:20-29) under --save_dir. Under a launcher
(`python -m torch.distributed.run --nproc-per-node N -m mllm_sparse_retrieval_amd search ...`, the counterpart of
`deepspeed --num_gpus=4 src/search.py`, scripts/search_sparse.sh:14) `search` is the reference's DP over queries
(src/search.py:180-182): every rank opens the index on its own GPU, searches its DistributedSampler shard of the
queries, and only recall fractions are gathered (src/metrices.py:86-100). `eval` is the recall reporter on its own.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from types import SimpleNamespace


def _cmd_encode(a):
    import numpy as np

    from . import workloads

    if a.synthetic is None:
        sys.exit("encode: only --synthetic {flickr,coco} is available (the MLLM encoder is out of scope here)")
    if a.synthetic == "flickr":
        wl = workloads.flickr30k_t2i(n_images=a.n_images or 1000, seed=a.seed, threads=a.threads)
        name = "flickr"
    else:
        wl = workloads.flickr30k_t2i(n_images=a.n_images or 5000, n_terms=30000, seed=a.seed, threads=a.threads)
        name = "coco"
    out = a.sparse_output_dir
    os.makedirs(out, exist_ok=True)
    dp, dt, dw = wl.docs
    with open(os.path.join(out, f"corpus_{a.dataset_shard_index}.jsonl"), "w") as f:
        for i in range(len(dp) - 1):
            vec = {f"t{int(t)}": int(w) for t, w in zip(dt[dp[i]:dp[i + 1]], dw[dp[i]:dp[i + 1]])}
            f.write(json.dumps(dict(id=str(i), content="", vector=vec)) + "\n")
    qp, qt, qw = wl.queries
    with open(os.path.join(out, "query.tsv"), "w") as f:
        for i in range(len(qp) - 1):
            toks = " ".join(" ".join([f"t{int(t)}"] * int(w)) for t, w in zip(qt[qp[i]:qp[i + 1]], qw[qp[i]:qp[i + 1]]))
            if toks.strip():
                f.write(f"{i}\t{toks}\n")
    if a.dense_output_dir:  # dense reps in the reference's pickle layout (reps, lookup) (src/encode.py:405-410)
        import pickle

        os.makedirs(a.dense_output_dir, exist_ok=True)
        rng = np.random.default_rng(a.seed)
        n_docs, n_q = len(dp) - 1, len(qp) - 1
        p = rng.standard_normal((n_docs, a.dense_dim)).astype(np.float32)
        # planted signal: a caption's vector is its image's vector plus noise
        qv = p[np.arange(n_q) // 5] + 1.5 * rng.standard_normal((n_q, a.dense_dim)).astype(np.float32)
        p /= np.linalg.norm(p, axis=1, keepdims=True)
        with open(os.path.join(a.dense_output_dir, f"corpus_{a.dataset_shard_index}.pkl"), "wb") as f:
            pickle.dump((p, [str(i) for i in range(n_docs)]), f)
        with open(os.path.join(a.dense_output_dir, "query.pkl"), "wb") as f:
            pickle.dump((qv, [str(i) for i in range(n_q)]), f)
    with open(os.path.join(out, "qrels.csv"), "w") as f:  # flickr csv schema (src/dataset.py:86-102)
        f.write("imgid,filename,caption,sentid\n")
        for i in range(len(qp) - 1):
            f.write(f"{i // 5},{i // 5}.jpg,,{i}\n")
    print(f"encode: {len(dp) - 1} docs, {len(qp) - 1} queries ({name}-shape, synthetic) -> {out}")


def _cmd_index(a):
    from .index import build_index_from_jsonl

    out = os.path.join(a.index, "msr.idx") if a.index else None
    if a.index:
        os.makedirs(a.index, exist_ok=True)
    t0 = time.time()
    path = build_index_from_jsonl(a.input, out, threads=a.threads, tile_docs=a.tile_docs)
    print(f"index: {path} ({os.path.getsize(path) / 1e6:.1f} MB) in {time.time() - t0:.2f}s")


def _cmd_vectors(a):
    """Doc vectors out of the index (msr_doc_vectors) as jsonl in the encode format (src/encode.py:351-359)."""
    import numpy as np

    from .index import SparseIndex, index_file_of

    if a.docids is not None and a.docids_file is not None:
        sys.exit("vectors: give --docids or --docids_file, not both")
    out = a.output or os.path.join(a.sparse_index if os.path.isdir(a.sparse_index) else os.path.dirname(a.sparse_index),
                                   "vectors.jsonl")
    with SparseIndex(index_file_of(a.sparse_index), device=a.device) as ix:
        if a.docids is None and a.docids_file is None:
            # every doc, whole tiles at a time; a chunk is sized by the average row to stay well below 2^32 entries
            ords = np.arange(ix.n_docs, dtype=np.uint32)
            avg = max(1, -(-ix.n_postings // max(1, ix.n_docs)))
            chunk = ix.tile_docs * max(1, (1 << 26) // (avg * ix.tile_docs))
        else:
            if a.docids is not None:
                ids = [d for d in a.docids.split(",") if d]
            else:
                with open(a.docids_file, encoding="utf-8") as f:
                    ids = [ln.strip() for ln in f if ln.strip()]
            ord_of = {d: o for o, d in enumerate(ix.docid_table().tolist())}
            unknown = [d for d in ids if d not in ord_of]
            if unknown:
                print(f"vectors: not in the index: {', '.join(unknown)}", file=sys.stderr)
            ords = np.asarray([ord_of[d] for d in ids if d in ord_of], dtype=np.uint32)
            chunk = 1 << 16
        toks, n_entries = {}, 0
        with open(out, "w", encoding="utf-8") as f:
            for c0 in range(0, len(ords), chunk):
                part = ords[c0:c0 + chunk]
                d_ptr, term, weight = ix.doc_vectors(part)
                n_entries += len(term)
                for t in np.unique(term).tolist():
                    if t not in toks:
                        toks[t] = ix.term_str(t)
                d_ptr, term, weight = d_ptr.tolist(), term.tolist(), weight.tolist()
                for e, docid in enumerate(ix.docids(part)):
                    vec = {toks[term[j]]: weight[j] for j in range(d_ptr[e], d_ptr[e + 1])}
                    f.write(json.dumps(dict(id=docid, content="", vector=vec)) + "\n")
    print(f"Doc vectors: {len(ords)} docs, {n_entries} entries -> {out}")


def read_queries(path):
    """query.tsv (`id\\ttok tok tok`, src/encode.py:418-424) or query jsonl ({"id","vector"}) -> (ids, strings)."""
    ids, texts = [], []
    with open(path, encoding="utf-8") as f:
        if path.endswith((".jsonl", ".json")):
            for line in f:
                if line.strip():
                    o = json.loads(line)
                    ids.append(str(o["id"]))
                    texts.append(" ".join(" ".join([t] * int(v)) for t, v in o["vector"].items() if int(v) > 0))
        else:
            for line in f:
                line = line.rstrip("\n")
                if line:
                    qid, _, text = line.partition("\t")
                    ids.append(qid)
                    texts.append(text)
    return ids, texts


def normalize_rows(q):
    """F.normalize(q, dim=-1) as the reference applies it to the query reps (src/search.py:342), in f32."""
    import numpy as np

    q = np.asarray(q, dtype=np.float32)
    return q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-12)


def parse_alphas(text, alpha):
    """--alphas `0,0.1,...,1` -> the floats in the order given, --alpha appended when it is not among them (compared as
    f32, which is what the library fuses with). Raises ValueError with the reason."""
    import math

    import numpy as np

    from ._cabi import MSR_SWEEP_MAX_ALPHAS

    parts = [x.strip() for x in str(text).split(",")]
    if not any(parts):
        raise ValueError("the list is empty")
    out = []
    for x in parts:
        try:
            v = float(x)
        except ValueError:
            raise ValueError(f"{x!r} is not a number") from None
        if not math.isfinite(v) or abs(v) > float(np.finfo(np.float32).max):   # (the library fuses in f32)
            raise ValueError(f"{x!r} is not finite")
        out.append(v)
    if not any(np.float32(v) == np.float32(alpha) for v in out):
        out.append(float(alpha))
    if len(out) > MSR_SWEEP_MAX_ALPHAS:
        raise ValueError(f"{len(out)} alphas (--alpha included), at most MSR_SWEEP_MAX_ALPHAS = {MSR_SWEEP_MAX_ALPHAS}")
    return out


def _check_sweep_args(a):
    """The contradictions of `search --alphas`: every one exits with its own message before any index is opened."""
    from ._cabi import MSR_KMAX

    if getattr(a, "alphas", None) is None:
        if getattr(a, "sweep_runs", False):
            sys.exit("search: --sweep_runs writes one run per alpha of --alphas: give --alphas")
        return
    if a.sparse_index is None or a.passage_reps is None:
        sys.exit("search: --alphas sweeps the hybrid search on the GPU: give both --passage_reps and --sparse_index")
    # (their own contradictions are _check_fusion_deep_args' / _check_fusion_filtered_args'; no depth or tile limit)
    if getattr(a, "fusion_deep", False) or getattr(a, "fusion_filtered", False):
        try:
            a.sweep_alphas = parse_alphas(a.alphas, a.alpha)
        except ValueError as e:
            sys.exit(f"search: --alphas {a.alphas!r}: {e}")
        return
    for flag, on, why in (
            ("--host_fusion", a.host_fusion, "the sweep is one msr_hybrid_sweep call on the GPU; fuse() on the host has no sweep"),
            ("--fusion_union", getattr(a, "fusion_union", False), "the sweep keeps the union on the device and returns the best "
                                                                  "--fusion_k docs per alpha"),
            ("--deep", getattr(a, "deep", False), f"the sweep holds at most MSR_KMAX = {MSR_KMAX} docs per list"),
            ("--doc_sets / --query_sets", getattr(a, "doc_sets", None) or getattr(a, "query_sets", None),
             "msr_hybrid_sweep takes no doc sets (the filtered sweep is --fusion_filtered --alphas)"),
            ("--ranks", getattr(a, "ranks", False), "a fused rank beyond the depth is not defined"),
            ("--explain", getattr(a, "explain", None) is not None, "--explain is the sparse-only route")):
        if on:
            sys.exit(f"search: --alphas does not combine with {flag}: {why}")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        sys.exit("search: --alphas runs in one process (no launcher, WORLD_SIZE = 1)")
    if not 1 <= a.depth <= MSR_KMAX:
        sys.exit(f"search: --alphas needs --depth in [1, MSR_KMAX = {MSR_KMAX}] (got {a.depth}; it is not clamped under "
                 "this flag)")
    try:
        a.sweep_alphas = parse_alphas(a.alphas, a.alpha)
    except ValueError as e:
        sys.exit(f"search: --alphas {a.alphas!r}: {e}")
    from .index import SparseIndex

    with SparseIndex(_index_path(a.sparse_index), device=-1) as meta:  # host-side metadata only: no GPU work
        if meta.tile_docs not in (4096, 8192):
            sys.exit(f"search: --alphas needs an index with 4096- or 8192-doc tiles, {a.sparse_index} has "
                     f"{meta.tile_docs}: rebuild it with --tile_docs 4096 / 8192")


def _check_fusion_deep_args(a):
    """The contradictions of `search --fusion_deep`: every one exits with its own message before any index is opened; the
    warning about a union that may be cut goes to stderr."""
    from ._cabi import MSR_DEEP_KMAX

    if not getattr(a, "fusion_deep", False):
        return
    if a.sparse_index is None or a.passage_reps is None:
        sys.exit("search: --fusion_deep is the hybrid search on the GPU: give both --passage_reps and --sparse_index")
    for flag, on, why in (
            ("--host_fusion", a.host_fusion, "--fusion_deep is one msr_hybrid_deep call on the GPU, --host_fusion the "
                                             "reference's loop with fuse() on the host"),
            ("--fusion_union", getattr(a, "fusion_union", False), "--fusion_deep returns the whole union itself, from "
                                                                  "msr_hybrid_deep instead of msr_hybrid_search_union"),
            ("--deep", getattr(a, "deep", False), "--deep is the sparse-only, dense-only and --host_fusion routes; "
                                                  "--fusion_deep takes --depth up to 16384 by itself"),
            ("--doc_sets / --query_sets", getattr(a, "doc_sets", None) or getattr(a, "query_sets", None),
             "filtered deep hybrid search is --fusion_filtered (one msr_hybrid_deep_filtered call)"),
            ("--ranks", getattr(a, "ranks", False), "a fused rank beyond the depth is not defined"),
            ("--explain", getattr(a, "explain", None) is not None, "--explain is the sparse-only route")):
        if on:
            sys.exit(f"search: --fusion_deep does not combine with {flag}: {why}")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        sys.exit("search: --fusion_deep runs in one process (no launcher, WORLD_SIZE = 1)")
    if not 1 <= a.depth <= MSR_DEEP_KMAX:
        sys.exit(f"search: --fusion_deep needs --depth in [1, MSR_DEEP_KMAX = {MSR_DEEP_KMAX}] (got {a.depth}; it is not "
                 "clamped under this flag)")
    if 2 * a.depth > MSR_DEEP_KMAX:
        print(f"search: WARNING: --fusion_deep --depth {a.depth}: a fused union can hold 2 x depth = {2 * a.depth} docs, "
              f"fusion.trec at most MSR_DEEP_KMAX = {MSR_DEEP_KMAX} per query; a larger union is cut after its best "
              f"{MSR_DEEP_KMAX} docs and the run reports how many queries were cut", file=sys.stderr)


def _check_fusion_filtered_args(a):
    """The contradictions of `search --fusion_filtered`: every one exits with its own message before any index is opened;
    the warning about a union that may be cut goes to stderr."""
    from ._cabi import MSR_DEEP_KMAX

    if not getattr(a, "fusion_filtered", False):
        return
    if a.sparse_index is None or a.passage_reps is None:
        sys.exit("search: --fusion_filtered is the filtered hybrid search on the GPU: give both --passage_reps and "
                 "--sparse_index")
    if not (getattr(a, "doc_sets", None) and getattr(a, "query_sets", None)):
        sys.exit("search: --fusion_filtered needs both --doc_sets FILE (docid<TAB>set) and --query_sets FILE (qid<TAB>set)")
    for flag, on, why in (
            ("--host_fusion", a.host_fusion, "--fusion_filtered is one msr_hybrid_deep_filtered call on the GPU, "
                                             "--host_fusion two filtered lists and fuse() on the host"),
            ("--fusion_union", getattr(a, "fusion_union", False), "--fusion_filtered returns the whole union itself; "
                                                                  "msr_hybrid_search_union takes no doc sets"),
            ("--fusion_deep", getattr(a, "fusion_deep", False), "--fusion_deep is the unfiltered call (msr_hybrid_deep); "
                                                                "--fusion_filtered alone takes --depth up to 16384"),
            ("--deep", getattr(a, "deep", False), "--deep is the sparse-only, dense-only and --host_fusion routes; "
                                                  "--fusion_filtered takes --depth up to 16384 by itself"),
            ("--ranks", getattr(a, "ranks", False), "a fused rank beyond the depth is not defined"),
            ("--explain", getattr(a, "explain", None) is not None, "--explain is the sparse-only route")):
        if on:
            sys.exit(f"search: --fusion_filtered does not combine with {flag}: {why}")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        sys.exit("search: --fusion_filtered runs in one process (no launcher, WORLD_SIZE = 1)")
    if not 1 <= a.depth <= MSR_DEEP_KMAX:
        sys.exit(f"search: --fusion_filtered needs --depth in [1, MSR_DEEP_KMAX = {MSR_DEEP_KMAX}] (got {a.depth}; it is "
                 "not clamped under this flag)")
    if 2 * a.depth > MSR_DEEP_KMAX:
        print(f"search: WARNING: --fusion_filtered --depth {a.depth}: a fused union can hold 2 x depth = {2 * a.depth} docs, "
              f"fusion.trec at most MSR_DEEP_KMAX = {MSR_DEEP_KMAX} per query; a larger union is cut after its best "
              f"{MSR_DEEP_KMAX} docs and the run reports how many queries were cut", file=sys.stderr)


def _check_search_args(a):
    """Argument checks of `search` that need no index and no GPU."""
    from ._cabi import MSR_DEEP_KMAX, MSR_KMAX

    if a.sparse_index is None and a.passage_reps is None:
        sys.exit("search: give --sparse_index (sparse or hybrid search) and/or --passage_reps (dense search)")
    _check_fusion_filtered_args(a)
    _check_fusion_deep_args(a)
    _check_sweep_args(a)
    deep = bool(getattr(a, "deep", False))
    if deep:
        if not 1 <= a.depth <= MSR_DEEP_KMAX:
            sys.exit(f"search: --deep needs --depth in [1, MSR_DEEP_KMAX = {MSR_DEEP_KMAX}] (got {a.depth})")
        if getattr(a, "fusion_union", False) or getattr(a, "hybrid_f32", False):
            sys.exit("search: --deep does not combine with --fusion_union / --hybrid_f32: the fused GPU calls hold at most "
                     f"MSR_KMAX = {MSR_KMAX} docs per list; deep hybrid search is --host_fusion --deep (two deep lists, "
                     "fuse() on the host)")
        if a.sparse_index is not None and a.passage_reps is not None and not a.host_fusion:
            sys.exit("search: hybrid --deep needs --host_fusion (two deep lists per query and the reference's fuse() on the "
                     f"host); the fused GPU route holds at most MSR_KMAX = {MSR_KMAX} docs per list")
    if a.sparse_index is None and not deep and not 1 <= a.depth <= MSR_KMAX:
        sys.exit(f"search: dense-only --depth must be in [1, MSR_KMAX = {MSR_KMAX}] (got {a.depth})")
    if getattr(a, "ranks", False):
        if a.passage_reps is not None and a.sparse_index is not None:
            sys.exit("search: --ranks ranks on one route, sparse (--sparse_index alone) or dense (--passage_reps alone): a "
                     "fused score depends on the depth lists, so a rank beyond the depth is not defined; drop "
                     "--passage_reps or --sparse_index")
        if not a.qrels:
            sys.exit("search: --ranks ranks every query's judged docs and needs --qrels")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            sys.exit("search: --ranks runs in one process (no launcher, WORLD_SIZE = 1)")
    if getattr(a, "explain", None) is not None:
        from ._cabi import MSR_EXPLAIN_MAX_TARGETS

        if a.passage_reps is not None:
            sys.exit("search: --explain is the sparse-only route (the doc weights come from the sparse index alone): drop "
                     "--passage_reps")
        if not 1 <= a.explain <= MSR_EXPLAIN_MAX_TARGETS:
            sys.exit(f"search: --explain N needs 1 <= N <= MSR_EXPLAIN_MAX_TARGETS = {MSR_EXPLAIN_MAX_TARGETS} "
                     f"(got {a.explain})")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            sys.exit("search: --explain runs in one process (no launcher, WORLD_SIZE = 1)")
    if (getattr(a, "doc_sets", None) or getattr(a, "query_sets", None)) and not getattr(a, "fusion_filtered", False):
        if not (a.doc_sets and a.query_sets):
            sys.exit("search: filtered search needs both --doc_sets FILE (docid<TAB>set) and --query_sets FILE (qid<TAB>set)")
        if deep or getattr(a, "ranks", False) or getattr(a, "explain", None) is not None:
            sys.exit("search: --doc_sets / --query_sets do not combine with --deep, --ranks or --explain: filtered deep "
                     "lists and filtered ranks are not served (filter a --deep run on the host instead)")
        if a.sparse_index is not None and a.passage_reps is not None and not a.host_fusion:
            sys.exit("search: filtered hybrid search needs --host_fusion (two filtered lists per query and the reference's "
                     "fuse() on the host, --depth <= 1024) or --fusion_filtered (one msr_hybrid_deep_filtered call on the "
                     "GPU, --depth up to 16384, --alphas); the other fused GPU hybrid calls take no doc sets")
        if getattr(a, "fusion_union", False):
            sys.exit("search: --doc_sets / --query_sets do not combine with --fusion_union (a fused GPU hybrid call)")
        if not 1 <= a.depth <= MSR_KMAX:
            sys.exit(f"search: filtered search needs --depth in [1, MSR_KMAX = {MSR_KMAX}] (got {a.depth})")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            sys.exit("search: --doc_sets / --query_sets run in one process (no launcher, WORLD_SIZE = 1)")
    if getattr(a, "hybrid_f32", False):
        if a.use_gpu:
            sys.exit("search: --hybrid_f32 and --use_gpu contradict each other (--use_gpu is the reference's fp16 GPU "
                     "index, --hybrid_f32 its f32 CPU index)")
        if a.sparse_index is None or a.passage_reps is None:
            sys.exit("search: --hybrid_f32 applies to hybrid search: give both --passage_reps and --sparse_index")
    if getattr(a, "fusion_union", False):
        if a.host_fusion:
            sys.exit("search: --fusion_union and --host_fusion contradict each other (--fusion_union is one "
                     "msr_hybrid_search_union call on the GPU, --host_fusion the reference's loop with fuse() on the host)")
        if a.sparse_index is None or a.passage_reps is None:
            sys.exit("search: --fusion_union applies to hybrid search: give both --passage_reps and --sparse_index")
        if not 1 <= a.depth <= MSR_KMAX:
            sys.exit(f"search: --fusion_union needs --depth in [1, MSR_KMAX = {MSR_KMAX}] (got {a.depth}; it is not "
                     "clamped under this flag): lower --depth, or use --host_fusion")
        from .index import SparseIndex

        with SparseIndex(_index_path(a.sparse_index), device=-1) as meta:  # host-side metadata only: no GPU work
            if meta.tile_docs not in (4096, 8192):
                sys.exit(f"search: --fusion_union needs an index with 4096- or 8192-doc tiles, {a.sparse_index} has "
                         f"{meta.tile_docs}: rebuild it with --tile_docs 4096 / 8192, or use --host_fusion")


def _index_path(sparse_index):
    """--sparse_index names the directory the index step wrote (its `index` entry) or the index itself."""
    inner = os.path.join(sparse_index, "index")
    return inner if os.path.isdir(inner) else sparse_index


def _cmd_search(a):
    _check_search_args(a)
    from .fusion import write_trec_run
    from .qrels import CrossModalQrels
    from .recall import RecallMetrics
    from .run import get_run_dict, sparse_search
    from .searcher import JWhiteSpaceAnalyzer, LuceneImpactSearcher

    dense_retriever = p_reps = p_lookup = q_reps_by_id = None
    if a.passage_reps is not None:  # dense side of the hybrid search (src/search.py:227-237)
        import glob

        import numpy as np

        from .run import pickle_load, search_queries

        files = sorted(glob.glob(os.path.join(a.passage_reps, "corpus*.pkl")))
        if not files:
            sys.exit(f"search: no corpus*.pkl under {a.passage_reps}")
        p_reps, p_lookup = pickle_load(files[0])     # files written by this package's own encode step
        q_reps, q_lookup = pickle_load(os.path.join(a.passage_reps, "query.pkl"))
        q_reps_by_id = {str(i): r for i, r in zip(q_lookup, q_reps)}
    dense_only = a.sparse_index is None
    # one process per GPU under a launcher (src/search.py:115-129); gloo carries the recall fractions only
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    if world > 1:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if not dist.is_initialized():
            dist.init_process_group("gloo")
        a.device = int(os.environ.get("LOCAL_RANK", "0"))
        if os.environ.get("MSR_SHARE_GPU"):  # rehearsal on a box with fewer GPUs than ranks: ranks share the devices
            import torch

            a.device %= max(torch.cuda.device_count(), 1)
    if dense_only:  # scripts/search_dense.sh: the ids of query.pkl in file order, or those --queries lists, in its order
        searcher = None
        qids = [str(x) for x in q_lookup]
        if a.queries:
            wanted = read_queries(a.queries)[0]
            missing = [x for x in wanted if x not in q_reps_by_id]
            if missing:
                sys.exit(f"search: {len(missing)} ids of {a.queries} have no vector in query.pkl (first: {missing[0]})")
            qids = wanted
        texts = [""] * len(qids)
    else:
        searcher = LuceneImpactSearcher(_index_path(a.sparse_index), None, device=a.device, deep=bool(getattr(a, "deep", False)))
        searcher.set_analyzer(JWhiteSpaceAnalyzer())
        qids, texts = read_queries(a.queries or os.path.join(a.sparse_index, "query.tsv"))
    n_queries = len(qids)
    if world > 1:  # the reference's DistributedSampler split, padding included (src/search.py:180-182)
        from .sampler import distributed_sampler_indices

        pos = distributed_sampler_indices(n_queries, world, rank)
        if not a.compat_denominator:  # every query once: drop the padded repeats
            pos = [p for j, p in enumerate(pos) if rank + j * world < n_queries]
        qids, texts = [qids[p] for p in pos], [texts[p] for p in pos]
    bs = a.batch_size if a.batch_size > 0 else len(qids)
    args = SimpleNamespace(depth=a.depth, threads=a.threads, query_type=a.query_type)
    sparse_run, dense_run, fusion_run = {}, {}, {}
    args.batch_size, args.quiet = a.batch_size, True
    ds = dense_ranks = None
    d_args = args  # what the dense side of --host_fusion searches with
    if dense_only and getattr(a, "ranks", False):  # the judged rows go through the same open index as the search
        ds = CrossModalQrels(a.qrels, a.dataset_name)
    t0 = time.time()
    filtered = bool(getattr(a, "doc_sets", None))
    sweep = None
    if getattr(a, "fusion_filtered", False):  # ONE msr_hybrid_deep_filtered call over the whole query file
        sweep = {} if getattr(a, "alphas", None) is not None else None
        sparse_run, dense_run, fusion_run = _hybrid_deep_on_gpu(a, searcher, p_reps, p_lookup, q_reps_by_id, qids, texts, sweep,
                                                                filtered=True)
    elif filtered:  # sparse-only, dense-only or --host_fusion: one filtered call per side over the whole query file
        sparse_run, dense_run, fusion_run = _filtered_search(a, searcher, p_reps, p_lookup, q_reps_by_id, qids, texts)
    elif dense_only:
        dense_run, dense_ranks = _dense_only_search(a, p_reps, p_lookup, q_reps_by_id, qids, ds)
    elif p_reps is not None and not a.host_fusion:
        # Hybrid on the GPU (the default): this rank's WHOLE query shard in one msr_hybrid_search call — sparse scores,
        # both depth lists, the reference's fusion (src/hybrid.py:32-53) and the top --fusion_k never leave HBM.
        sweep = {} if getattr(a, "alphas", None) is not None else None
        route = _hybrid_deep_on_gpu if getattr(a, "fusion_deep", False) else _hybrid_on_gpu
        sparse_run, dense_run, fusion_run = route(a, searcher, p_reps, p_lookup, q_reps_by_id, qids, texts, sweep)
    else:
        if p_reps is not None:  # --host_fusion: the reference's own structure, batch by batch (src/search.py:455-461)
            from .dense import FaissFlatSearcher

            dense_retriever = FaissFlatSearcher(p_reps, device=a.device, precision="f32" if getattr(a, "hybrid_f32", False) else "fp16",
                                                deep=bool(getattr(a, "deep", False)))
            dense_retriever.add(p_reps)
            if getattr(a, "deep", False):  # a deep list never asks for more rows than the index holds
                d_args = SimpleNamespace(**vars(args))
                d_args.depth = min(a.depth, len(p_lookup))
        for i in range(0, len(qids), bs):
            scores, rankings = sparse_search(searcher, texts[i:i + bs], qids[i:i + bs], args)
            sparse_run.update(get_run_dict(qids[i:i + bs], scores, rankings, a.remove_query))
            if dense_retriever is not None:
                q = np.stack([q_reps_by_id[x] for x in qids[i:i + bs]])
                q = q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-12)    # F.normalize, src/search.py:342
                d_scores, d_ids = search_queries(dense_retriever, q, p_lookup, d_args)
                dense_run.update(get_run_dict(qids[i:i + bs], d_scores, d_ids, a.remove_query))
        if dense_retriever is not None:
            from .fusion import fuse

            fusion_run = fuse([dense_run, sparse_run], [a.alpha, 1 - a.alpha])         # src/search.py:455-461
    dt = time.time() - t0
    if not a.quiet:
        print(f"search: {len(qids)} queries in {dt:.3f}s ({len(qids) / max(dt, 1e-9):.0f} q/s end-to-end incl. host)")
    if a.save_dir:
        os.makedirs(a.save_dir, exist_ok=True)
        sfx = f".rank{rank}" if world > 1 else ""
        if getattr(a, "sweep_runs", False):
            for x, run in zip(sweep["alphas"], _sweep_runs(sweep, qids)):
                write_trec_run(run, os.path.join(a.save_dir, f"fusion.alpha_{x:g}.trec"))
        if not dense_only:  # (dense-only search writes the dense run alone: no sparse.trec, no fusion.trec)
            write_trec_run(sparse_run, os.path.join(a.save_dir, "sparse.trec" + sfx), name="sparse")
        if dense_run or dense_only:
            write_trec_run(dense_run, os.path.join(a.save_dir, "dense.trec" + sfx), name="dense")
        if dense_run and not dense_only:
            write_trec_run(fusion_run, os.path.join(a.save_dir, "fusion.trec" + sfx))
        if world > 1:  # rank 0 joins the per-rank files (one node, shared directory)
            dist.barrier()
            if rank == 0:
                for name in ("sparse.trec", "dense.trec", "fusion.trec"):
                    parts = [os.path.join(a.save_dir, f"{name}.rank{r}") for r in range(world)]
                    missing = [p for p in parts if not os.path.exists(p)]
                    if missing and len(missing) < len(parts):  # (all missing: that run was not produced at all)
                        print(f"search: WARNING: {name} not joined, rank files missing (one node and a shared --save_dir "
                              f"are assumed): {missing}", file=sys.stderr)
                    if not missing:
                        done = set()  # queries an earlier rank's file already holds (the sampler's padded repeats)
                        with open(os.path.join(a.save_dir, name), "w") as out:
                            for p in parts:
                                mine = set()
                                for line in open(p):
                                    qid = line.split(" ", 1)[0]
                                    if qid in done:
                                        continue
                                    mine.add(qid)
                                    out.write(line)
                                done |= mine
                        for p in parts:
                            os.remove(p)
    if a.qrels:
        ds = ds or CrossModalQrels(a.qrels, a.dataset_name)
        if getattr(a, "alphas", None) is not None:
            _report_sweep(a, sweep, ds, qids)
        m = RecallMetrics(ds, dense_run, sparse_run, fusion_run, p_lookup or [], qids, args,
                          denominator=None if (a.compat_denominator or world == 1) else n_queries)
        m.sort_and_count()
        m.all_gather_object()
        m.print_recall()
    if dense_ranks is not None:
        _report_dense_ranks(a, dense_ranks)
    elif getattr(a, "ranks", False):
        _report_exact_ranks(a, searcher, ds, qids, texts)
    if getattr(a, "explain", None) is not None:
        _report_explain(a, searcher, ds, qids, texts, sparse_run)
    if searcher is not None:
        searcher.close()
    if world > 1:
        dist.barrier()


def _filtered_search(a, searcher, p_reps, p_lookup, q_reps_by_id, qids, texts):
    """search --doc_sets FILE --query_sets FILE: every query searches only the docs of its set (a query without a line
    in --query_sets is unfiltered; a doc in no set belongs to no set). Sparse side: ONE batch_search_filtered call
    (msr_search_filtered); dense side: ONE DenseIndex.search_filtered call (msr_dense_search_filtered) with the sets over
    the rows of p_lookup, precision as on the unfiltered routes; with both (--host_fusion) the two filtered lists go
    through the reference's fuse(). A doc id the searched index does not know is an error. Returns the three run dicts."""
    import numpy as np

    from .filters import read_doc_sets, read_query_sets
    from .run import get_run_dict

    doc_sets, query_set = read_doc_sets(a.doc_sets), read_query_sets(a.query_sets)
    for qid in qids:
        if qid in query_set and query_set[qid] not in doc_sets:
            sys.exit(f"search: query {qid} names doc set {query_set[qid]!r}, which {a.doc_sets} does not define")
    sparse_run, dense_run, fusion_run = {}, {}, {}
    if searcher is not None:
        try:
            by_qid = searcher.batch_search_filtered(texts, qids, a.depth, doc_sets, query_set)
        except ValueError as e:
            sys.exit(f"search: {a.doc_sets}: {e}")
        sparse_run = get_run_dict(qids, [[h.score for h in by_qid[x]] for x in qids],
                                  [[h.docid for h in by_qid[x]] for x in qids], a.remove_query)
    if p_reps is not None:
        from .dense import DenseIndex

        row_of = {}
        for r, x in enumerate(p_lookup):
            row_of.setdefault(str(x), []).append(r)
        names = list(doc_sets)
        member = np.zeros((len(names), len(p_lookup)), dtype=bool)
        for s_i, name in enumerate(names):
            for d in doc_sets[name]:
                if str(d) not in row_of:
                    sys.exit(f"search: {a.doc_sets}: doc set {name!r}: no dense row carries doc id {d!r}")
                member[s_i, row_of[str(d)]] = True
        col = {name: s_i for s_i, name in enumerate(names)}
        q_set = np.asarray([col[query_set[x]] if x in query_set else -1 for x in qids], dtype=np.int32)
        q = normalize_rows(np.stack([q_reps_by_id[x] for x in qids])) if qids else np.zeros((0, p_reps.shape[1]), np.float32)
        if searcher is None:
            precision = "fp16" if a.use_gpu else "f32"
        else:
            precision = "f32" if getattr(a, "hybrid_f32", False) else "fp16"
        dix = DenseIndex(p_reps, device=a.device, precision=precision)
        try:
            d_scores, d_idx = dix.search_filtered(q, min(a.depth, dix.n), member, q_set)
        finally:
            dix.close()
        lookup = [str(x) for x in p_lookup]
        rows = [[j for j in d_idx[i].tolist() if j >= 0] for i in range(len(qids))]  # (a set smaller than the depth)
        dense_run = get_run_dict(qids, [d_scores[i, :len(rows[i])] for i in range(len(qids))],   # (f32, as unfiltered)
                                 [[lookup[j] for j in rows[i]] for i in range(len(qids))], a.remove_query)
        if searcher is not None:
            from .fusion import fuse

            fusion_run = fuse([dense_run, sparse_run], [a.alpha, 1 - a.alpha])
    return sparse_run, dense_run, fusion_run


def _sweep_runs(sweep, qids):
    """One fused run per alpha of a sweep, in the layout of _hybrid_on_gpu's fusion_run."""
    table = sweep["table"]
    for ords, fs, cnt in zip(sweep["ords"], sweep["scores"], sweep["n"]):
        fs_rows = fs.tolist()
        yield {qid: dict(zip(table[ords[i, :cnt[i]]].tolist(), fs_rows[i][:cnt[i]])) for i, qid in enumerate(qids)}


def _report_sweep(a, sweep, ds, qids):
    """search --alphas with --qrels: one line per alpha with the fusion recalls RecallMetrics reports for that alpha's
    lists (recall.sweep_recall: doc ids and targets compared as ints like src/metrices.py:33,41-44, the same denominator)
    and, with --save_dir, fusion.sweep.tsv: alpha, r@1, r@5, r@10, r@100, r@200, in the order given."""
    from .recall import RECALL_KS, sweep_recall

    def as_int(x):
        try:
            return int(x)
        except (TypeError, ValueError):
            return str(x)

    ord_of = {as_int(d): o for o, d in enumerate(sweep["table"].tolist())}
    targets = []
    for qid in qids:
        t = ds.get_target(qid, a.query_type)
        t = t if isinstance(t, list) else [t]
        targets.append([ord_of[as_int(x)] for x in t if as_int(x) in ord_of])
    counts = sweep_recall(sweep["ords"], sweep["n"], targets, RECALL_KS)
    denom = max(len(qids), 1)
    rows = []
    for x, c in zip(sweep["alphas"], counts.tolist()):
        r = [v / denom for v in c]
        rows.append((x, r))
        print("Fusion/Hybrid sweep alpha {:g}: r@1 {}, r@5 {}, r@10 {}, r@100 {}, r@200 {}".format(x, *r))
    if a.save_dir:
        os.makedirs(a.save_dir, exist_ok=True)
        with open(os.path.join(a.save_dir, "fusion.sweep.tsv"), "w") as f:
            for x, r in rows:
                f.write("\t".join([f"{x:g}"] + [repr(v) for v in r]) + "\n")


def _report_exact_ranks(a, searcher, ds, qids, texts):
    """search --ranks: the exact rank of every query's judged docs from ONE rank_docs call over the whole query file
    (no depth limit, so MRR / MedR / MeanR are exact), --remove_query honoured as get_run_dict does. Prints one line and,
    with --save_dir, writes sparse.ranks.tsv: qid, docid, rank, score per (query, target); rank 0 = not a hit or the
    query's own doc, rank -1 = the index does not hold that doc id."""
    import numpy as np

    from .ranks import rank_metrics

    targets = []
    for qid in qids:
        t = ds.get_target(qid, a.query_type)
        targets.append([str(x) for x in t] if isinstance(t, list) else [str(t)])
    res = searcher.batch_rank(texts, qids, targets, remove_query=a.remove_query)
    ranks, t_ptr, missing = [], [0], 0
    for qid, row in res.items():
        ranks.extend(r for _, r, _ in row if r is not None)
        missing += sum(1 for _, r, _ in row if r is None)
        t_ptr.append(len(ranks))
    m = rank_metrics(np.asarray(ranks, np.int64), np.asarray(t_ptr, np.int64), searcher.num_docs)
    rc = m["recall"]
    print("Sparse exact ranks: r@1 {}, r@5 {}, r@10 {}, r@100 {}, r@200 {}, mrr {}, medr {}, meanr {}, unranked {}, "
          "missing {}".format(rc[1], rc[5], rc[10], rc[100], rc[200], m["mrr"], m["medr"], m["meanr"], m["n_unranked"],
                              missing))
    if a.save_dir:
        with open(os.path.join(a.save_dir, "sparse.ranks.tsv"), "w") as f:
            for qid, row in res.items():
                for d, r, sc in row:
                    f.write(f"{qid}\t{d}\t{-1 if r is None else r}\t{0 if sc is None else sc}\n")


def _report_explain(a, searcher, ds, qids, texts, sparse_run):
    """search --explain N: the per-token addends of the first N hits of every query (after --remove_query's filter) and,
    with --qrels, of its judged docs as well (deduplicated), from ONE explain_docs call over the whole query file.
    Prints one line and, with --save_dir, writes sparse.explain.tsv (explain.tsv_lines: qid, docid, position, judged,
    score, token, q_w, d_w, contribution; one line per matched token)."""
    from ._cabi import MSR_EXPLAIN_MAX_TARGETS
    from .explain import write_tsv

    listed, hits_of, judged_of = [], [], []
    for qid in qids:
        hits = list(sparse_run[qid]["docs"])  # in rank order (get_run_dict keeps the hit order)
        docs = hits[:a.explain]
        judged = []
        if ds is not None:
            t = ds.get_target(qid, a.query_type)
            judged = [str(x) for x in t] if isinstance(t, list) else [str(t)]
            docs += [d for d in dict.fromkeys(judged) if d not in docs]
        if len(docs) > MSR_EXPLAIN_MAX_TARGETS:
            sys.exit(f"search: --explain: query {qid} would list {len(docs)} docs ({a.explain} hits + its judged docs), "
                     f"at most MSR_EXPLAIN_MAX_TARGETS = {MSR_EXPLAIN_MAX_TARGETS}: lower --explain")
        listed.append(docs)
        hits_of.append({d: i + 1 for i, d in enumerate(hits)})
        judged_of.append(set(judged))
    res = searcher.batch_explain(texts, qids, listed)
    records, missing = [], 0
    for i, qid in enumerate(qids):
        for d, _score, rows in res[qid]:
            if rows is None:  # the index does not hold that doc id
                missing += 1
                continue
            records.append((qid, d, hits_of[i].get(d, 0), d in judged_of[i], rows))
    print("Sparse explain: {} (query, doc) pairs, {} matched tokens, missing {}".format(
        len(records), sum(len(r[4]) for r in records), missing))
    if a.save_dir:
        write_tsv(os.path.join(a.save_dir, "sparse.explain.tsv"), records)


def _dense_rank_targets(a, ds, p_lookup, qids):
    """The judged rows of every query for search --ranks on the dense route: ds.get_target ids mapped to dense rows through
    p_lookup (first occurrence wins). -> (per query [(docid, row or None)], t_ptr, t_row, self_row or None); a judged id
    without a row stays in the listing (reported as missing) and is not ranked."""
    import numpy as np

    from ._cabi import MSR_DENSE_RANK_MAX_TARGETS

    row_of = {}
    for r, x in enumerate(p_lookup):
        row_of.setdefault(str(x), r)
    listing, t_ptr, t_row = [], [0], []
    for qid in qids:
        t = ds.get_target(qid, a.query_type)
        docs = [str(x) for x in t] if isinstance(t, list) else [str(t)]
        listing.append([(d, row_of.get(d)) for d in docs])
        t_row.extend(r for _, r in listing[-1] if r is not None)
        if len(t_row) - t_ptr[-1] > MSR_DENSE_RANK_MAX_TARGETS:
            sys.exit(f"search: --ranks: query {qid} has {len(t_row) - t_ptr[-1]} judged rows, at most "
                     f"MSR_DENSE_RANK_MAX_TARGETS = {MSR_DENSE_RANK_MAX_TARGETS}")
        t_ptr.append(len(t_row))
    self_row = np.asarray([row_of.get(x, -1) for x in qids], dtype=np.int32) if a.remove_query else None
    return listing, np.asarray(t_ptr, np.int64), np.asarray(t_row, np.uint32), self_row


def _dense_only_search(a, p_reps, p_lookup, q_reps_by_id, qids, ds=None):
    """search --passage_reps without --sparse_index (scripts/search_dense.sh): this rank's WHOLE query shard in one
    DenseIndex.search call. Precision follows the reference (src/search.py:254-270): the f32 flat index it searches on
    the CPU by default, fp16 storage with --use_gpu. Returns the dense run in the layout of get_run_dict
    (src/search.py:66-82), --remove_query applied there as the reference does, and, with `ds` (search --ranks), the exact
    ranks of every query's judged rows from ONE rank_rows call on the same index and the same normalised query matrix
    (no depth limit; --remove_query names the row whose id equals the query id as self_row), else None."""
    import numpy as np

    from ._cabi import MSR_KMAX
    from .dense import DenseIndex, keys_to_f32
    from .run import get_run_dict

    q = normalize_rows(np.stack([q_reps_by_id[x] for x in qids])) if qids else np.zeros((0, p_reps.shape[1]), np.float32)
    targets = _dense_rank_targets(a, ds, p_lookup, qids) if ds is not None else None
    ranked = None
    dix = DenseIndex(p_reps, device=a.device, precision="fp16" if a.use_gpu else "f32")
    try:
        depth = min(a.depth, dix.n)
        if getattr(a, "deep", False) and depth > MSR_KMAX:
            d_scores, d_idx = dix.search_deep(q, depth)
        else:
            d_scores, d_idx = dix.search(q, depth)
        if targets is not None:
            listing, t_ptr, t_row, self_row = targets
            ranks, keys = dix.rank_rows(q, t_ptr, t_row, self_row)
            ranked = dict(qids=qids, listing=listing, t_ptr=t_ptr, ranks=ranks, scores=keys_to_f32(keys), n_rows=dix.n)
    finally:
        dix.close()
    lookup = np.asarray([str(x) for x in p_lookup], dtype=object)
    return get_run_dict(qids, d_scores, lookup[d_idx], a.remove_query), ranked


def _report_dense_ranks(a, r):
    """search --ranks on the dense route: prints one line (the figures of ranks.rank_metrics over the exact ranks) and,
    with --save_dir, writes dense.ranks.tsv: qid, docid, rank, f32 score (repr of the float: reads back bit-exact) per
    (query, judged id); rank 0 = the query's own row, rank -1 (score 0) = no dense row carries that id."""
    from .ranks import rank_metrics

    m = rank_metrics(r["ranks"], r["t_ptr"], r["n_rows"])
    missing = sum(1 for rows in r["listing"] for _, row in rows if row is None)
    rc = m["recall"]
    print("Dense exact ranks: r@1 {}, r@5 {}, r@10 {}, r@100 {}, r@200 {}, mrr {}, medr {}, meanr {}, unranked {}, "
          "missing {}".format(rc[1], rc[5], rc[10], rc[100], rc[200], m["mrr"], m["medr"], m["meanr"], m["n_unranked"],
                              missing))
    if a.save_dir:
        with open(os.path.join(a.save_dir, "dense.ranks.tsv"), "w") as f:
            e = 0
            for qid, rows in zip(r["qids"], r["listing"]):
                for d, row in rows:
                    if row is None:
                        f.write(f"{qid}\t{d}\t-1\t0\n")
                    else:
                        f.write(f"{qid}\t{d}\t{int(r['ranks'][e])}\t{float(r['scores'][e])!r}\n")
                        e += 1


def _hybrid_on_gpu(a, searcher, p_reps, p_lookup, q_reps_by_id, qids, texts, sweep=None):
    """search --passage_reps on the GPU: ONE msr_hybrid_search call for the fused run; the sparse and the dense run the
    reference also reports (src/metrices.py:105-126) come from one whole-shard call each. Returns the three run dicts in
    the reference's layouts (src/search.py:66-82; the fused run without the 'docs' level, src/hybrid.py:32-53).
    --hybrid_f32: an f32 DenseIndex and hybrid_search_f32 (the reference's f32 flat index) instead of fp16.
    --fusion_union: ONE msr_hybrid_search_union call instead, from which all three runs come (fusion.union_to_runs): the
    fused run holds the WHOLE union as the reference's does, and nothing is scored a second time.
    --alphas (sweep: a dict to fill): ONE msr_hybrid_sweep call (dense.hybrid_sweep) for the whole query file at every alpha
    of a.sweep_alphas, k = min(--fusion_k, 2 x depth); --alpha's slice is the fused run, so nothing is fused twice, and
    `sweep` receives every slice (alphas, ords, scores, n, table).
    Difference to --host_fusion: the fused run holds the best --fusion_k docs of the union (the recall reporter reads
    200, src/metrices.py:9), and an exact tie of two DENSE scores at the depth boundary goes to the lower doc ordinal
    instead of the lower row (include/msr.h)."""
    import numpy as np

    from .dense import DenseIndex, hybrid_search, hybrid_search_f32, hybrid_search_union, hybrid_sweep, row_to_ordinal
    from .fusion import union_to_runs
    from .run import get_run_dict

    ix = searcher.index
    depth = min(a.depth, 1024)
    k_f = max(1, min(a.fusion_k, 1024))
    q_ptr, q_term, q_w = ix.encode_queries(texts)
    q = np.stack([q_reps_by_id[x] for x in qids]).astype(np.float32) if qids else np.zeros((0, p_reps.shape[1]), np.float32)
    q = q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-12)                # F.normalize, src/search.py:342
    f32 = bool(getattr(a, "hybrid_f32", False))
    dix = DenseIndex(p_reps, device=ix.device, precision="f32" if f32 else "fp16")
    hybrid = hybrid_search_f32 if f32 else hybrid_search
    try:
        table = ix.docid_table()
        ord_of = {d: o for o, d in enumerate(table.tolist())}
        r2o = np.asarray([ord_of[str(x)] for x in p_lookup], dtype=np.uint32)
        self_ord = np.asarray([ord_of.get(x, -1) for x in qids], dtype=np.int32) if a.remove_query else None
        drop = searcher.min_idf >= 0 if searcher.drop_df_eq_n is None else bool(searcher.drop_df_eq_n)
        if getattr(a, "fusion_union", False):
            ords, fs, cnt, src, su, de, rng, _ = hybrid_search_union(ix, dix, q_ptr, q_term, q_w, q, depth, a.alpha, r2o,
                                                                     self_ord, drop_df_eq_n=drop,
                                                                     with_lists=not a.fusion_only)
            return union_to_runs(qids, table, ords, cnt, fs, src, su, de, rng)
        if sweep is not None:
            alphas = list(a.sweep_alphas)
            s_ords, s_fs, s_cnt, _ = hybrid_sweep(ix, dix, q_ptr, q_term, q_w, q, depth, max(1, min(a.fusion_k, 2 * depth)),
                                                  alphas, r2o, self_ord, drop_df_eq_n=drop)
            sweep.update(alphas=alphas, ords=s_ords, scores=s_fs, n=s_cnt, table=table)
            at = [np.float32(x) == np.float32(a.alpha) for x in alphas].index(True)
            ords, fs, cnt = s_ords[at], s_fs[at], s_cnt[at]
        else:
            ords, fs, cnt, _ = hybrid(ix, dix, q_ptr, q_term, q_w, q, depth, k_f, a.alpha, r2o, self_ord, drop_df_eq_n=drop)
        fs_rows = fs.tolist()
        fusion_run = {qid: dict(zip(table[ords[i, :cnt[i]]].tolist(), fs_rows[i][:cnt[i]])) for i, qid in enumerate(qids)}
        sparse_run, dense_run = {}, {}
        if not a.fusion_only:
            o, f, _, c = ix.search_csr(q_ptr, q_term, q_w, depth, drop_df_eq_n=drop)
            f_rows = f.tolist()
            sparse_run = get_run_dict(qids, [f_rows[i][:c[i]] for i in range(len(qids))],
                                      [table[o[i, :c[i]]].tolist() for i in range(len(qids))], a.remove_query)
            d_scores, d_idx = dix.search(q, min(depth, dix.n))
            lookup = np.asarray([str(x) for x in p_lookup], dtype=object)
            dense_run = get_run_dict(qids, d_scores, lookup[d_idx], a.remove_query)
    finally:
        dix.close()
    return sparse_run, dense_run, fusion_run


def _ordinal_doc_sets(a, ord_of, qids, n_docs):
    """--doc_sets / --query_sets as msr_hybrid_deep_filtered takes them: (packed sets over doc ordinals, q_set int32 [nq]).
    Doc ids map to ordinals as on the filtered sparse route: a doc id the index does not hold and a set name --doc_sets does
    not define are errors, a query without a line is unfiltered (-1), a doc listed in no set belongs to no set."""
    import numpy as np

    from .filters import read_doc_sets, read_query_sets, sets_from_ordinals

    doc_sets, query_set = read_doc_sets(a.doc_sets), read_query_sets(a.query_sets)
    names = list(doc_sets)
    col = {name: s for s, name in enumerate(names)}
    lists = []
    for name in names:
        unknown = [str(d) for d in doc_sets[name] if str(d) not in ord_of]
        if unknown:
            sys.exit(f"search: {a.doc_sets}: doc set {name!r}: the index does not hold doc id {unknown[0]!r}"
                     + (f" (and {len(unknown) - 1} more)" if len(unknown) > 1 else ""))
        lists.append([ord_of[str(d)] for d in doc_sets[name]])
    q_set = np.full(len(qids), -1, dtype=np.int32)
    for i, qid in enumerate(qids):
        name = query_set.get(qid)
        if name is None:
            continue
        if name not in col:
            sys.exit(f"search: query {qid} names doc set {name!r}, which {a.doc_sets} does not define")
        q_set[i] = col[name]
    return sets_from_ordinals(lists, n_docs), q_set


def _hybrid_deep_on_gpu(a, searcher, p_reps, p_lookup, q_reps_by_id, qids, texts, sweep=None, filtered=False):
    """search --fusion_deep: ONE msr_hybrid_deep call (dense.hybrid_deep) over the whole query file, --depth up to
    MSR_DEEP_KMAX. All three runs come from it: both depth lists as get_run_dict builds them (min / max over the unfiltered
    list, the query's own doc skipped under --remove_query) and the WHOLE fused union at --alpha, up to
    k = min(2 x depth, MSR_DEEP_KMAX) docs per query (--fusion_k is not read). With --alphas (sweep: a dict to fill) the same
    call fuses at every alpha of a.sweep_alphas and `sweep` receives every slice, as on the msr_hybrid_sweep route.
    --hybrid_f32: an f32 DenseIndex instead of fp16. Prints how many queries' unions were cut at k (out_members).
    A dense tie AT the depth boundary goes to the lower doc ordinal (include/msr.h), not to the lower row as --host_fusion's;
    inside the written dense list, docs of equal score stand by row as there.
    search --fusion_filtered (filtered=True): ONE msr_hybrid_deep_filtered call (dense.hybrid_deep_filtered) instead, with the
    doc sets of --doc_sets / --query_sets over doc ordinals; everything else, the outputs included, is the same."""
    import numpy as np

    from ._cabi import MSR_DEEP_KMAX
    from .dense import DenseIndex, hybrid_deep, hybrid_deep_filtered
    from .run import get_run_dict

    ix = searcher.index
    depth = a.depth
    k = min(2 * depth, MSR_DEEP_KMAX)
    q_ptr, q_term, q_w = ix.encode_queries(texts)
    q = np.stack([q_reps_by_id[x] for x in qids]).astype(np.float32) if qids else np.zeros((0, p_reps.shape[1]), np.float32)
    q = q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-12)                # F.normalize, src/search.py:342
    dix = DenseIndex(p_reps, device=ix.device, precision="f32" if getattr(a, "hybrid_f32", False) else "fp16")
    try:
        table = ix.docid_table()
        ord_of = {d: o for o, d in enumerate(table.tolist())}
        r2o = np.asarray([ord_of[str(x)] for x in p_lookup], dtype=np.uint32)
        self_ord = np.asarray([ord_of.get(x, -1) for x in qids], dtype=np.int32) if a.remove_query else None
        drop = searcher.min_idf >= 0 if searcher.drop_df_eq_n is None else bool(searcher.drop_df_eq_n)
        alphas = list(a.sweep_alphas) if sweep is not None else [a.alpha]
        if filtered:
            bits, q_set = _ordinal_doc_sets(a, ord_of, qids, ix.n_docs)
            res = hybrid_deep_filtered(ix, dix, q_ptr, q_term, q_w, q, depth, k, alphas, r2o, bits, q_set, self_ord,
                                       drop_df_eq_n=drop, with_lists=not a.fusion_only)
        else:
            res = hybrid_deep(ix, dix, q_ptr, q_term, q_w, q, depth, k, alphas, r2o, self_ord, drop_df_eq_n=drop,
                              with_lists=not a.fusion_only)
    finally:
        dix.close()
    if sweep is not None:
        sweep.update(alphas=alphas, ords=res.ords, scores=res.scores, n=res.n, table=table)
    at = [np.float32(x) == np.float32(a.alpha) for x in alphas].index(True)
    ords, fs_rows, cnt = res.ords[at], res.scores[at].tolist(), res.n[at]
    fusion_run = {qid: dict(zip(table[ords[i, :cnt[i]]].tolist(), fs_rows[i][:cnt[i]])) for i, qid in enumerate(qids)}
    cut = int((res.members > cnt.astype(np.int64)).sum())
    if cut or not a.quiet:
        print(f"search: --fusion_{'filtered' if filtered else 'deep'}: {cut} of {len(qids)} queries have a fused union of more than k = {k} docs (cut after "
              f"the best {k}); largest union {int(res.members.max(initial=0))} docs")
    sparse_run, dense_run = {}, {}
    if not a.fusion_only:
        s_rows = res.sparse_u32.astype(np.float32).tolist()      # (float)u32, as the sparse search returns its scores
        sparse_run = get_run_dict(qids, [s_rows[i][:res.sparse_n[i]] for i in range(len(qids))],
                                  [table[res.sparse_ords[i, :res.sparse_n[i]]].tolist() for i in range(len(qids))], a.remove_query)
        # dense.trec lists docs of equal score by ROW, as the dense search and --host_fusion do (the call lists them by
        # ordinal): one stable sort per list by (score descending, row ascending)
        row_of = np.empty(len(r2o), dtype=np.uint64)
        row_of[r2o] = np.arange(len(r2o), dtype=np.uint64)
        live = np.arange(res.dense_ords.shape[1])[None, :] < res.dense_n[:, None]
        bits = np.ascontiguousarray(res.dense).view(np.uint32)
        d_key = np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint64)
        comp = ((np.uint64(0xFFFFFFFF) - d_key) << np.uint64(32)) | row_of[np.where(live, res.dense_ords, 0)]
        order = np.argsort(np.where(live, comp, np.uint64(0xFFFFFFFFFFFFFFFF)), axis=1, kind="stable")
        d_ords, d_sc = np.take_along_axis(res.dense_ords, order, axis=1), np.take_along_axis(res.dense, order, axis=1)
        dense_run = get_run_dict(qids, [d_sc[i, :res.dense_n[i]] for i in range(len(qids))],
                                 [table[d_ords[i, :res.dense_n[i]]] for i in range(len(qids))], a.remove_query)
    return sparse_run, dense_run, fusion_run


def _cmd_eval(a):
    """Standalone recall reporter over TREC runs: sparse/dense/fusion.trec (src/hybrid.py:8-29
    format) + the dataset csv -> the reference's print-out (src/metrices.py:103-137). Default denominator: the true
    number of queries; --compat-denominator replays --world_size ranks of the reference (DistributedSampler shards,
    padded repeats searched and counted twice, len(lookup_indices) * world, src/metrices.py:92)."""
    from .fusion import read_trec_run
    from .qrels import CrossModalQrels
    from .recall import replay_ranks

    def load(explicit, name):
        path = explicit or (os.path.join(a.runs_dir, name) if a.runs_dir else None)
        return read_trec_run(path) if path and os.path.exists(path) else {}

    sparse_run, dense_run = load(a.sparse_run, "sparse.trec"), load(a.dense_run, "dense.trec")
    fusion_run = {q: v["docs"] for q, v in load(a.fusion_run, "fusion.trec").items()}  # no 'docs' level (src/metrices.py:70-73)
    if not (sparse_run or dense_run or fusion_run):
        sys.exit("eval: no run file found (--runs_dir with sparse.trec / dense.trec / fusion.trec, or --sparse_run ...)")
    ds = CrossModalQrels(a.qrels, a.dataset_name)
    # the query universe in dataset order: captions ('full' mode) or images ('single'), src/dataset.py:104-110
    query_ids = ds.text_id_list if a.query_type == "text" else ds.img_id_list
    if a.queries:
        query_ids = read_queries(a.queries)[0]
    # the reference prints len(look_up) = the number of corpus passages (src/metrices.py:106): take it from
    # --n_passages, else from the dataset's passage universe, else from the docs the dense run happens to hold
    if a.n_passages:
        look_up = list(range(a.n_passages))
    else:
        universe = ds.img_id_list if a.query_type == "text" else ds.text_id_list
        look_up = list(universe) or sorted({d for v in dense_run.values() for d in v["docs"]})
    args = SimpleNamespace(query_type=a.query_type)
    world = a.world_size if a.compat_denominator else 1
    m = replay_ranks(ds, dense_run, sparse_run, fusion_run, look_up, query_ids, args, world, compat=a.compat_denominator)
    m.print_recall()
    return m


def main(argv=None):
    ap = argparse.ArgumentParser(prog="mllm_sparse_retrieval_amd")
    sub = ap.add_subparsers(dest="cmd", required=True)

    e = sub.add_parser("encode")
    e.add_argument("--synthetic", choices=["flickr", "coco"])
    e.add_argument("--sparse_output_dir", default="./sparse_output/")
    e.add_argument("--dense_output_dir", default=None)
    e.add_argument("--dense_dim", type=int, default=256)
    e.add_argument("--dataset_shard_index", type=int, default=0)
    e.add_argument("--n_images", type=int, default=0)
    e.add_argument("--seed", type=int, default=1)
    e.add_argument("--threads", type=int, default=16)
    e.set_defaults(fn=_cmd_encode)

    i = sub.add_parser("index")
    i.add_argument("--input", required=True)
    i.add_argument("--index", default=None)
    i.add_argument("--threads", type=int, default=16)
    i.add_argument("--tile_docs", type=int, default=0)
    for flag in ("--collection", "--generator"):  # pyserini flags of scripts/sparse_index.sh, accepted and ignored
        i.add_argument(flag, default=None)
    i.add_argument("--impact", action="store_true")
    i.add_argument("--pretokenized", action="store_true")
    i.set_defaults(fn=_cmd_index)

    s = sub.add_parser("search")
    s.add_argument("--sparse_index", default=None,
                   help="sparse index directory (sparse search; hybrid with --passage_reps)")
    s.add_argument("--passage_reps", default=None,
                   help="dense reps directory (corpus*.pkl + query.pkl); without --sparse_index: dense-only search "
                        "(scripts/search_dense.sh), f32 unless --use_gpu")
    s.add_argument("--depth", type=int, default=1000)
    s.add_argument("--threads", type=int, default=1)
    s.add_argument("--batch_size", type=int, default=128)
    s.add_argument("--alpha", type=float, default=0.5)
    s.add_argument("--remove_query", action="store_true")
    s.add_argument("--query_type", default="text")
    s.add_argument("--dataset_name", default="flickr")
    s.add_argument("--save_dir", default=None)
    s.add_argument("--quiet", action="store_true")
    s.add_argument("--use_gpu", action="store_true",
                   help="dense-only search: fp16 passage storage like the reference's faiss GPU clone (default f32, "
                        "its CPU index); ignored by the sparse and hybrid routes (hybrid precision: --hybrid_f32)")
    s.add_argument("--queries", default=None)
    s.add_argument("--qrels", default=None)
    s.add_argument("--device", type=int, default=0)
    s.add_argument("--host_fusion", action="store_true",
                   help="hybrid: the reference's own structure (dense + sparse lists per batch, fuse() on the host) "
                        "instead of one msr_hybrid_search call over the whole query file")
    s.add_argument("--hybrid_f32", action="store_true",
                   help="hybrid: f32 dense side (the reference's default f32 flat index, no --use_gpu) on both the GPU "
                        "route (msr_hybrid_search_f32) and --host_fusion, instead of fp16 storage; needs --passage_reps "
                        "and --sparse_index, refused with --use_gpu")
    s.add_argument("--fusion_k", type=int, default=1000, help="hybrid on the GPU: docs kept of each query's fused union "
                                                              "(<= 1024); ignored under --fusion_union")
    s.add_argument("--fusion_union", action="store_true",
                   help="hybrid on the GPU: ONE msr_hybrid_search_union call for the whole query file; fusion.trec holds "
                        "the WHOLE union of both depth lists (up to 2 x --depth docs per query, as the reference's fuse() "
                        "keeps them) and sparse.trec / dense.trec come from the same call; with --hybrid_f32 on the f32 "
                        "handle; --depth <= 1024, not with --host_fusion, --fusion_k is ignored")
    s.add_argument("--fusion_only", action="store_true", help="hybrid on the GPU: skip the separate sparse and dense runs (with or without --fusion_union; "
                                                                   "the fused run then feeds the recall report only: fusion.trec is written beside a dense run)")
    s.add_argument("--alphas", default=None, metavar="A,B,...",
                   help="hybrid on the GPU: sweep the fusion weight, e.g. 0,0.1,0.2,0.3,0.4,0.5,0.6,0.7,0.8,0.9,1 (at most 64 "
                        "values, --alpha is added if absent): ONE msr_hybrid_sweep call scores the whole query file once and "
                        "fuses it at every alpha, k = min(--fusion_k, 2 x --depth); with --qrels prints one 'Fusion/Hybrid "
                        "sweep alpha' line per alpha and writes fusion.sweep.tsv under --save_dir; --alpha's slice is the "
                        "usual fused run; honours --hybrid_f32, --remove_query, --fusion_only; --depth <= 1024, 4096- or "
                        "8192-doc tiles; not with --host_fusion, --fusion_union, --deep, --doc_sets / --query_sets, --ranks, "
                        "--explain or under a launcher")
    s.add_argument("--sweep_runs", action="store_true",
                   help="with --alphas and --save_dir: also write fusion.alpha_{a}.trec, the fused run of every alpha")
    s.add_argument("--deep", action="store_true",
                   help="lists beyond 1024: lifts --depth to [1, MSR_DEEP_KMAX = 16384] on the sparse-only route "
                        "(msr_search_deep), the dense-only route (msr_dense_search_deep; fp16 with --use_gpu, else f32) and, "
                        "with --host_fusion, the hybrid route (two deep lists per query, fuse() on the host: fusion.trec "
                        "holds the whole union); refused on the fused GPU hybrid routes, with --fusion_union and with "
                        "--hybrid_f32; depths up to 1024 take the usual calls")
    s.add_argument("--fusion_deep", action="store_true",
                   help="hybrid on the GPU beyond 1024: ONE msr_hybrid_deep call over the whole query file with --depth in "
                        "[1, 16384]; writes sparse.trec, dense.trec and fusion.trec, the WHOLE fused union (up to "
                        "min(2 x --depth, 16384) docs per query; --fusion_k is not read), and reports how many queries' "
                        "unions were cut (possible when 2 x --depth > 16384: a warning says so); with --alphas the same "
                        "call fuses at every alpha (fusion.sweep.tsv, --sweep_runs: fusion.alpha_{a}.trec); needs "
                        "--passage_reps and --sparse_index; honours --hybrid_f32, --use_gpu, --remove_query, --fusion_only; "
                        "not with --host_fusion, --fusion_union, --deep, --doc_sets / --query_sets (that is "
                        "--fusion_filtered), --ranks, --explain or under a launcher")
    s.add_argument("--fusion_filtered", action="store_true",
                   help="filtered hybrid on the GPU: --fusion_deep among the docs of each query's set, ONE "
                        "msr_hybrid_deep_filtered call over the whole query file; needs --doc_sets FILE --query_sets FILE, "
                        "--passage_reps and --sparse_index; --depth in [1, 16384], not clamped (a warning when 2 x --depth > "
                        "16384); writes what --fusion_deep writes; works with --alphas and --sweep_runs, --hybrid_f32, "
                        "--use_gpu, --remove_query, --fusion_only; not with --host_fusion, --fusion_union, --fusion_deep, "
                        "--deep, --ranks, --explain or under a launcher")
    s.add_argument("--doc_sets", default=None, metavar="FILE",
                   help="filtered search: TSV lines docid<TAB>set naming doc sets; with --query_sets every query searches "
                        "only the docs of its set (msr_search_filtered / msr_dense_search_filtered): sparse-only, dense-only "
                        "and --host_fusion routes, and with --fusion_filtered the hybrid route on the GPU "
                        "(msr_hybrid_deep_filtered); refused on the other GPU-fused hybrid routes and with --deep, --ranks, "
                        "--explain")
    s.add_argument("--query_sets", default=None, metavar="FILE",
                   help="filtered search: TSV lines qid<TAB>set; a query without a line is unfiltered")
    s.add_argument("--ranks", action="store_true",
                   help="sparse search (--sparse_index alone) or dense search (--passage_reps alone, f32 or --use_gpu): after "
                        "the search, the EXACT rank (no depth limit) of every query's --qrels docs from one msr_rank_docs / "
                        "msr_dense_rank_rows call; prints recall, MRR, MedR, MeanR and writes sparse.ranks.tsv / "
                        "dense.ranks.tsv under --save_dir; honours --remove_query; not on the hybrid route (--passage_reps "
                        "with --sparse_index) or under a launcher")
    s.add_argument("--explain", type=int, default=None, metavar="N",
                   help="sparse search: after the search, WHY the first N hits of every query (1 <= N <= 64; after "
                        "--remove_query's filter) and, with --qrels, its judged docs score what they score: per-token "
                        "query weight x doc weight from one msr_explain_docs call; writes sparse.explain.tsv under "
                        "--save_dir; not with --passage_reps or under a launcher")
    s.add_argument("--compat-denominator", "--compat_denominator", dest="compat_denominator", action="store_true",
                   help="multi-rank: keep the sampler's padded repeats and divide by len(shard) * world like the reference")
    s.set_defaults(fn=_cmd_search)

    v = sub.add_parser("eval")
    v.add_argument("--runs_dir", default=None)
    v.add_argument("--sparse_run", default=None)
    v.add_argument("--dense_run", default=None)
    v.add_argument("--fusion_run", default=None)
    v.add_argument("--qrels", required=True, help="dataset csv (data/flickr/flickr_test.csv schema, src/dataset.py:86-102)")
    v.add_argument("--dataset_name", default="flickr")
    v.add_argument("--query_type", default="text")
    v.add_argument("--n_passages", type=int, default=0, help="corpus size for the dense report's header line "
                                                            "(default: the dataset's passage universe)")
    v.add_argument("--queries", default=None, help="query.tsv giving the query universe / order (default: the csv's)")
    v.add_argument("--compat-denominator", "--compat_denominator", dest="compat_denominator", action="store_true")
    v.add_argument("--world_size", type=int, default=4, help="ranks to replay with --compat-denominator "
                                                             "(scripts/search_sparse.sh:14 uses 4)")
    v.set_defaults(fn=_cmd_eval)

    d = sub.add_parser("vectors", help="doc vectors out of the index as jsonl in the encode format (every doc, or the "
                                       "listed ones), read on the GPU by msr_doc_vectors")
    d.add_argument("--sparse_index", required=True)
    d.add_argument("--docids", default=None, help="comma-separated external doc ids (default: every doc, in ordinal order)")
    d.add_argument("--docids_file", default=None, help="one external doc id per line")
    d.add_argument("--output", default=None, help="default: <sparse_index>/vectors.jsonl")
    d.add_argument("--device", type=int, default=0)
    d.set_defaults(fn=_cmd_vectors)

    a = ap.parse_args(argv)
    a.fn(a)


if __name__ == "__main__":
    main()
