/*
 * msr.h — C-ABI of the MI355X-native learned-sparse retrieval scorer.
 *
 * This is the drop-in boundary for the reference's sparse search step. In the reference
 * (cjc20000323/mllm_sparse_retrieval) that step is three calls into pyserini/Anserini/Lucene:
 *
 *     LuceneImpactSearcher(index_dir, None)              src/search.py:273
 *     searcher.set_analyzer(JWhiteSpaceAnalyzer())       src/search.py:274-275
 *     searcher.batch_search(queries, qids, k, threads)   src/search.py:86-87
 *
 * plus the offline index build `python -m pyserini.index.lucene --impact --pretokenized`
 * (scripts/sparse_index.sh:12-18) over the jsonl written by src/encode.py:351-359,426.
 * Each entry point below names the reference interface it replaces.
 *
 * Conventions
 *   - plain C, no C++/torch types; every function returns 0 (MSR_OK) or a negative MSR_E_* code and
 *     never throws; msr_last_error() returns a thread-local message for the last failure.
 *   - the caller allocates every output array; the library owns only opaque handles and device buffers.
 *   - one in-flight call per handle (each index handle owns one HIP stream); handles are not thread-safe.
 *   - all integers little-endian, fixed width. Doc "ordinals" are ranks of the external doc-id strings in
 *     bytewise ascending order, so "lower ordinal wins a score tie" is the declared tie rule T1
 *      by construction.
 *   - scoring is exact unsigned 32-bit integer arithmetic on the GPU; a query whose worst-case score
 *     could exceed 2^32-1 is rejected with MSR_E_OVERFLOW rather than computed inexactly.
 *   - there is NO CPU scoring path in this library: searching a handle opened with device < 0, or on a
 *     machine without a usable HIP device, fails with MSR_E_NODEVICE.
 */
#ifndef MSR_H
#define MSR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSR_OK 0
#define MSR_E_INVAL (-1)    /* bad argument */
#define MSR_E_IO (-2)       /* file could not be read / written */
#define MSR_E_FORMAT (-3)   /* malformed jsonl line or index file */
#define MSR_E_NOMEM (-4)    /* host or device allocation failed */
#define MSR_E_NODEVICE (-5) /* no HIP device bound to this handle */
#define MSR_E_HIP (-6)      /* a HIP runtime call failed */
#define MSR_E_OVERFLOW (-7) /* worst-case score of a query exceeds 2^32-1 */
#define MSR_E_RANGE (-8)    /* term id / weight / k outside the supported range */
#define MSR_E_COMM (-9)     /* RCCL failure */

/* search flags */
#define MSR_F_DROP_DF_EQ_N 1u /* drop query terms present in every doc (pyserini idf>min_idf filter, contract T3) */

#define MSR_KMAX 1024 /* largest supported k (reference default depth is 1000, src/arguments.py:59) */

typedef struct msr_index msr_index; /* an opened (optionally device-resident) inverted index */
typedef struct msr_batch msr_batch; /* a device-resident batch of CSR queries + its result buffers */

typedef struct msr_info {
    uint64_t n_docs;        /* docs in the whole index */
    uint64_t n_postings;    /* (term,doc) pairs with weight > 0 in the whole index */
    uint64_t n_vecs;        /* 16-byte posting vectors stored (postings + per-segment padding) */
    uint32_t n_terms;       /* dictionary size */
    uint32_t tile_docs;     /* docs per tile (accumulator tile held in LDS) */
    uint32_t n_tiles;       /* tiles in the whole index */
    uint32_t max_weight;    /* largest stored weight */
    uint32_t shard_tile0;   /* first tile resident on this handle */
    uint32_t shard_ntiles;  /* tiles resident on this handle */
    int32_t device;         /* HIP device ordinal, or -1 */
    uint32_t n_dense;       /* terms stored in the dense head */
    uint32_t term_lo;       /* term-range shards: terms [term_lo, term_hi) are resident (else 0 .. n_terms) */
    uint32_t term_hi;
    uint64_t resident_bytes; /* bytes of the index (segment table + postings + dense head) this handle holds in HBM */
} msr_info;

/* ---- index build: replaces scripts/sparse_index.sh:12-18 (pyserini.index.lucene --impact --pretokenized) ----
 * Reads every *.jsonl / *.json file of `jsonl_dir` (lines {"id":…,"content":…,"vector":{tok:int}} as written by
 * src/encode.py:351-359,426) and writes one index file. tile_docs = 0 picks the default (8192); supported: 4096, 8192, 12288, 16384, 32768. */
int msr_index_build(const char* jsonl_dir, const char* out_path, int threads, uint32_t tile_docs);

/* Process-wide build options (set before building; not thread-safe):
 *   "dense_min_density" (default 0.4): a term with df >= density * n_docs is stored in the doc-major dense head
 *   "dense_max_terms"   (default 16, at most 32; 0 disables the dense head)
 *   "tie_order"         (default 0: doc ordinals = rank of the doc-id string, so a score tie goes to the bytewise lower
 *                        doc id, contract T1; 1: ordinals = input order, a tie goes to the doc indexed first) */
int msr_set_build_option(const char* key, double value);

/* Same index from a doc-major CSR already in memory (used by the synthetic encode step and the benchmark).
 * doc_ids / term_strs may be NULL: docs are then named by their decimal row number and terms by their decimal id. */
int msr_index_build_csr(const char* out_path, uint64_t n_docs, uint32_t n_terms, const uint64_t* doc_ptr,
                        const uint32_t* term_id, const uint32_t* weight, const char* const* doc_ids,
                        const char* const* term_strs, int threads, uint32_t tile_docs);

/* ---- open / close: replaces LuceneImpactSearcher(index_dir, None), src/search.py:273 ----
 * device >= 0 uploads the postings to that HIP device; device = -1 opens host-side metadata only
 * (dictionary, df, doc ids) — such a handle cannot search. */
int msr_index_open(const char* path, int device, msr_index** out);

/* Doc-range shard `shard` of `n_shards` (contiguous tile range): only that slice of the
 * postings is uploaded. Ordinals in results stay global. */
int msr_index_open_shard(const char* path, int device, int shard, int n_shards, msr_index** out);

/* Term-range shard `shard` of `n_shards` (the north star's partition, BASELINE.json configs[3]; no counterpart in the
 * reference, which opens one whole index per rank, src/search.py:216,273): term ranges are contiguous in term id and
 * balanced by postings; of every doc tile only the segments of the owned terms, the matching columns of the segment
 * table and the dense-head pairs that hold an owned term are uploaded. Such a handle serves the term-range protocol only
 * (msr_batch_create_termshard with the same shard / n_shards, msr_batch_search_termshard,
 * msr_search_termshard_emulated_handles); a plain msr_batch_create on it is refused. */
int msr_index_open_termshard(const char* path, int device, int shard, int n_shards, msr_index** out);

/* Closing an index releases the device buffers of every batch still alive on it and detaches those batches: they
 * fail with MSR_E_INVAL afterwards and msr_batch_destroy only frees the host object. */
void msr_index_close(msr_index* ix);
int msr_index_info(const msr_index* ix, msr_info* info);

/* token -> term id (-1 = not in the index vocabulary); the host-side half of pyserini's query encoding
 * that src/search.py:86-87 triggers. */
int msr_term_lookup(const msr_index* ix, const char* const* toks, int n, int32_t* term_ids);
int msr_term_df(const msr_index* ix, const int32_t* term_ids, int n, uint32_t* df);
int msr_term_str(const msr_index* ix, uint32_t term_id, const char** s);
/* external doc id of an ordinal: `hit.docid`, src/search.py:97. Borrowed pointer, valid until close. */
int msr_docid_str(const msr_index* ix, uint32_t ord, const char** s);

/* ---- search: replaces searcher.batch_search(queries, qids, k, threads), src/search.py:86-87 ----
 * Queries are CSR: query i owns entries [q_ptr[i], q_ptr[i+1]) of (q_term, q_w). Entries with q_term < 0
 * (out-of-vocabulary) or q_w <= 0 are ignored; duplicate terms add (src/search.py:419-422).
 * Outputs (row-major [nq][k]): doc ordinals, scores as f32 (`hit.score`), optional exact u32 scores,
 * and out_n[i] = number of hits of query i (only docs with score > 0 are hits, so out_n[i] <= k). The f32 score is
 * (float)u32, round to nearest even; slots past out_n[i] hold ordinal 0xFFFFFFFF and score 0 / 0.f. */
int msr_search_csr(msr_index* ix, const int64_t* q_ptr, const int32_t* q_term, const int32_t* q_w, int nq, int k,
                   uint32_t flags, uint32_t* out_doc_ord, float* out_score, uint32_t* out_score_u32,
                   int32_t* out_n);

/* ---- deep lists: the plain ranked list beyond MSR_KMAX, "the best 2 000 / 5 000 / 10 000 docs of every query". The
 * reference treats depth as a free integer (src/arguments.py:59, passed into batch_search at src/search.py:57,86);
 * rerankers, pooling and MedR-style analysis consume such lists. MSR_DEEP_KMAX is 16 384 because one row of 16 384
 * composite u64 keys is 128 KiB: it fits one workgroup's LDS on gfx950 (160 KiB per CU), so a single in-LDS sort is
 * possible. The scoring is the search's own accumulation (the exact u32 scores of every doc, dumped per tile); one
 * kernel, deep_select_rows, then takes the exact top-k of each query's score row.
 * Queries are CSR and normalised exactly as by msr_search_csr (MSR_F_DROP_DF_EQ_N honoured, the same MSR_E_OVERFLOW /
 * MSR_E_RANGE refusals). 1 <= k <= MSR_DEEP_KMAX, anything else is MSR_E_RANGE; k may exceed n_docs. Outputs are
 * row-major [nq][k] with the meaning and the padding of msr_search_csr: hits are the docs with score > 0, ordered by
 * score descending, lower ordinal first; out_n[i] = min(k, hits); slots past out_n[i] hold 0xFFFFFFFF / 0 / 0.f; the f32
 * score is (float)u32, round to nearest even. out_score_u32 may be NULL.
 * IDENTITIES: for k <= MSR_KMAX every output array is bit-equal to msr_search_csr at that k; for any k, columns
 * [0, min(k, 1024)) equal the search at k = 1024; the doc at column c < out_n[i] of row i has rank c + 1 from
 * msr_rank_docs on the same inputs with self_ord NULL.
 * Only a whole-index handle is served (doc-range and term-range shard handles: MSR_E_INVAL, as for msr_rank_docs); all
 * five tile sizes, with or without a dense head. ms (nullable) = HIP-event times summed over the passes of queries (the
 * score rows of one pass stay at or below 256 MiB): {the scoring launches, the deep selection}.
 * Argument errors are reported before any device work: MSR_E_INVAL for a null ix / q_ptr / out_doc_ord / out_score /
 * out_n, nq < 0 and a shard handle; then MSR_E_RANGE for k; then MSR_E_NODEVICE on a handle opened with device < 0 (the
 * CSR arrays themselves are checked with the normalisation, as by msr_search_csr). nq == 0 returns MSR_OK without a
 * launch. Measured against the staged search at k = 1000: DESIGN.md §5. */
#define MSR_DEEP_KMAX 16384 /* largest k of the deep calls */
int msr_search_deep(msr_index* ix, const int64_t* q_ptr, const int32_t* q_term, const int32_t* q_w, int nq, int k,
                    uint32_t flags, uint32_t* out_doc_ord, float* out_score, uint32_t* out_score_u32, int32_t* out_n,
                    float ms[2]);

/* ---- filtered search: "search, but only among these docs". Every query names one of the call's doc SETS and its hits are
 * the members of that set; Lucene does this with filter queries, which the reference never issues (its COCO 1K folds,
 * one modality of a mixed corpus, a reranker's candidate list above the 64 listed docs of msr_rank_docs, tombstones:
 * today each needs an index of its own).
 * DOC SETS. set_bits is [n_sets][W] with W = (n + 31) / 32 words, n = n_docs here (on the dense route below: the number
 * of rows, bits over ROW indices). Bit (o & 31) (bit 0 = LSB) of word (o >> 5) of row s says that doc o belongs to set
 * s. Bits at or above n in the last word are ignored (they cannot surface a padding doc). q_set[i] in [-1, n_sets) picks
 * the set of query i, -1 = the query is unfiltered. q_set may be NULL when n_sets is 0 (nothing is filtered) or 1 (every
 * query uses set 0). At most MSR_FILTER_MAX_SETS sets per call.
 * Queries are CSR and normalised exactly as by msr_search_csr (the same flags, the same MSR_E_OVERFLOW / MSR_E_RANGE
 * refusals). The hits of query i are the docs of its set with score > 0; order (score descending, lower ordinal first),
 * padding (0xFFFFFFFF / 0 / 0.f), the f32 image and out_n are those of msr_search_csr. 1 <= k <= MSR_KMAX. out_score_u32
 * may be NULL. ms (nullable) = HIP-event times of {the scoring launches including the stage-1 merge, the final merge}.
 * IDENTITIES: a full set, or q_set = -1, is bit-equal to msr_search_csr at that k; for any set the list equals the
 * unfiltered exact ranking (msr_search_deep at a k that covers every hit) with the non-members struck out, cut to k; the
 * lists of a set and of its complement partition the unfiltered hits.
 * The scores are the search's own accumulation (accumulate_tile / accumulate_tile_light); a kernel of its own,
 * score_tiles_filtered, masks the tile's scores with the set's bits before the unchanged selection, and a (tile, query)
 * whose set holds no doc of the tile leaves before accumulating. The call always takes the staged launches of
 * msr_batch_search: never the one-workgroup walk of small indexes and never the zero-copy path of small calls.
 * Only a whole-index handle is served (doc-range and term-range shard handles: MSR_E_INVAL, as for msr_search_deep).
 * Argument errors are reported before any device work, in this order: MSR_E_INVAL for a null ix / q_ptr / out_doc_ord /
 * out_score / out_n, nq < 0, n_sets < 0, a null set_bits with n_sets > 0, a null q_set with n_sets > 1 and a shard
 * handle; MSR_E_RANGE for k, for n_sets > MSR_FILTER_MAX_SETS and for a q_set entry outside [-1, n_sets); then
 * MSR_E_NODEVICE on a handle opened with device < 0 (the CSR arrays themselves are checked with the normalisation).
 * nq == 0 returns MSR_OK without a launch. Measured against the unfiltered search: DESIGN.md §5. */
#define MSR_FILTER_MAX_SETS 65536 /* doc sets of one filtered call */
int msr_search_filtered(msr_index* ix, const int64_t* q_ptr, const int32_t* q_term, const int32_t* q_w, int nq, int k,
                        uint32_t flags, const uint32_t* set_bits, int n_sets, const int32_t* q_set,
                        uint32_t* out_doc_ord, float* out_score, uint32_t* out_score_u32, int32_t* out_n, float ms[2]);

/* ---- exact ranks of listed docs: "where does this doc stand for this query", at any depth. Stands beside the ranked
 * lists the reference reads its hits from (src/search.py:86-99) and the recall counting over them (src/metrices.py);
 * there is NO counterpart call in the reference or in pyserini: a judged doc below the search depth is simply missing
 * there, so MedR / MeanR / MRR / Recall@k beyond the depth cannot be computed exactly from a run.
 * Queries are CSR and normalised exactly as by msr_search_csr (q_term < 0 and q_w <= 0 ignored, duplicate terms add,
 * MSR_F_DROP_DF_EQ_N honoured, the same MSR_E_OVERFLOW / MSR_E_RANGE refusals). The listed docs (targets) are CSR too:
 * query i owns entries [t_ptr[i], t_ptr[i+1]) of t_ord (doc ordinals; at most MSR_RANK_MAX_TARGETS per query, duplicates
 * allowed, none is fine). Both outputs are indexed like t_ord. With s(d) the exact u32 score of doc d for the query:
 *     out_score_u32 = s(t)
 *     out_rank      = 0 when s(t) == 0 (not a hit: no search returns it) or t == self_ord[i],
 *                     else 1 + #{ d != self_ord[i] : s(d) > s(t) or (s(d) == s(t) and d < t) }
 * i.e. the search path's key order (score descending, lower ordinal wins). self_ord (nullable; entries may be -1) names
 * the doc remove_query drops (src/search.py:72-74). With self_ord NULL and any k <= MSR_KMAX, t is in row i of
 * msr_search_csr(..., k) exactly when 1 <= rank <= k, at column rank - 1 with the same u32 score.
 * ms (nullable) = HIP-event times of {the gather launch(es): scores of the listed docs, tiles without one are not
 * touched; the count launch(es) over every (tile, query) plus the reduction}.
 * Only a whole-index handle is served: a doc-range or term-range shard handle is refused with MSR_E_INVAL (a rank
 * counts over every doc and needs every term). Argument errors are reported before the device is looked at:
 * MSR_E_INVAL for a null ix / q_ptr / t_ptr / output, nq < 0, a t_ptr that does not start at 0 or decreases;
 * MSR_E_RANGE for an ordinal or a self_ord entry >= n_docs and for more than MSR_RANK_MAX_TARGETS targets in one query;
 * then MSR_E_NODEVICE on a handle opened with device < 0. nq == 0 or no target at all returns MSR_OK without a launch. */
#define MSR_RANK_MAX_TARGETS 64 /* listed docs per query */
int msr_rank_docs(msr_index* ix, const int64_t* q_ptr, const int32_t* q_term, const int32_t* q_w, int nq, uint32_t flags,
                  const int64_t* t_ptr, const uint32_t* t_ord, const int32_t* self_ord, uint32_t* out_rank,
                  uint32_t* out_score_u32, float ms[2]);

/* ---- explain listed docs: "WHY does this doc score what it scores", the stored doc weight of every query term for
 * listed (query, doc) pairs. Counterpart: Lucene's IndexSearcher.explain(), which the reference never calls (none in
 * src/search.py; its src/sparse_statistic.py / src/score_statistic.py re-read the encoder output instead). The index is
 * tile-major inverted, there is no forward index: this call reads the addends out of the segments and the dense head on
 * the device, with kernels of its own that share no code with the accumulation of the search / rank path.
 * Queries and listed docs (targets) are CSR exactly as for msr_rank_docs (same query normalisation, same
 * MSR_E_OVERFLOW / MSR_E_RANGE refusals, at most MSR_EXPLAIN_MAX_TARGETS targets per query, duplicates allowed, none is
 * fine). out_doc_w is ragged: target entry e of query i(e) owns len_i = q_ptr[i+1] - q_ptr[i] consecutive slots from
 *     x_off(e) = sum over e' < e of len_i(e'),
 * and slot j of entry e belongs to input entry q_ptr[i] + j of the query (term tau, weight omega), listed doc t:
 *     out_doc_w[x_off(e) + j] = w(tau, t), the stored weight of tau in t, when the entry counts,
 *                               0 when t lacks tau or the entry does not count.
 * An entry counts when tau >= 0, omega > 0 and it is not dropped by MSR_F_DROP_DF_EQ_N; a repeated term gets the same
 * weight in each of its slots (duplicates add). out_cap = number of u32 the caller allocated, at least the sum of
 * len_i(e) over all target entries. IDENTITY: for every entry e,
 *     sum over j of max(omega_j, 0) * out_doc_w[x_off(e) + j]  ==  out_score_u32[e] of msr_rank_docs on the same inputs.
 * ms (nullable) = HIP-event time of the explain work on the stream {zeroing the output + the explain launch(es)}.
 * Only a whole-index handle is served (doc-range and term-range shard handles: MSR_E_INVAL); all five tile sizes, with
 * or without a dense head. Argument errors are reported before the device is looked at: MSR_E_INVAL for a null ix /
 * q_ptr / t_ptr / output (or q_term / q_w / t_ord with entries to read), nq < 0, a q_ptr that is negative or decreases,
 * a t_ptr that does not start at 0 or decreases, an out_cap below the sum above; MSR_E_RANGE for an ordinal >= n_docs
 * and for more than MSR_EXPLAIN_MAX_TARGETS targets in one query; then MSR_E_NODEVICE on a handle opened with
 * device < 0. nq == 0, no target at all or only zero-length queries return MSR_OK without a launch. There is no CPU
 * path. */
#define MSR_EXPLAIN_MAX_TARGETS 64 /* listed docs per query */
int msr_explain_docs(msr_index* ix, const int64_t* q_ptr, const int32_t* q_term, const int32_t* q_w, int nq,
                     uint32_t flags, const int64_t* t_ptr, const uint32_t* t_ord, uint32_t* out_doc_w, int64_t out_cap,
                     float ms[1]);

/* ---- doc vectors: "WHAT does this doc hold", every term of listed docs with its stored weight. Counterpart: Lucene's
 * IndexReader.getTermVector() (pyserini: IndexReader.get_document_vector(docid)), which the reference never calls (none
 * in src/search.py; its src/sparse_statistic.py re-reads the encoder output for the histograms of stored doc weights).
 * The index is tile-major inverted, there is no forward index: this call streams the postings of every tile that holds
 * a listed doc on the device, with kernels of its own, and returns the rows as a doc-major CSR.
 * t_ord holds n doc ordinals: any count, duplicates allowed, any mix of tiles, every doc of the index in one call is
 * fine. Listed entry e owns [out_ptr[e], out_ptr[e+1]) of (out_term, out_w): every term the doc holds with its stored
 * weight (1 .. 65535) in ASCENDING TERM ID; dense-head terms are merged into the same order and cannot be told from
 * segment terms; a repeated ordinal gets its own equal row. For an index built by msr_index_build_csr from rows sorted
 * by term, listing ordinal o returns exactly the input row of the doc that got ordinal o.
 * Sizing as msr_encode_queries: out_ptr (n + 1 entries) and *n_entries are always filled; out_term / out_w are filled
 * when cap >= *n_entries (call with cap = 0 and null arrays to size).
 * ms (nullable) = HIP-event times of {count pass, fill pass, ordering pass}; a pass that was not launched reports 0.
 * Argument errors are reported before the device is looked at: MSR_E_INVAL for a null ix / out_ptr / n_entries, for a
 * null t_ord with n > 0, n < 0, cap < 0, for null out_term / out_w with cap > 0; MSR_E_RANGE for an ordinal >= n_docs;
 * MSR_E_INVAL for a doc-range or term-range shard handle; then MSR_E_NODEVICE on a handle opened with device < 0.
 * n == 0 returns MSR_OK with out_ptr[0] = 0 and no launch. A total of 2^32 entries or more is MSR_E_RANGE (known after
 * the count pass; out_ptr and *n_entries are filled): split the list. There is no CPU path. */
int msr_doc_vectors(msr_index* ix, const uint32_t* t_ord, int64_t n, int64_t* out_ptr, uint32_t* out_term, uint32_t* out_w,
                    int64_t cap, int64_t* n_entries, float ms[3]);

/* Where the calling thread's last msr_search_csr spent its time, in microseconds: {query normalisation + device buffers
 * + upload enqueued, kernels enqueued, wait for the stream, download + copy out, release, the whole call, 0, 0}. Slots 6
 * and 7 (once HIP-event spans of the kernels) stay in the ABI and are always 0: the call records no events. The reference
 * calls batch_search with 4 queries at a time (scripts/search_sparse.sh:16): such a call is launch- and copy-latency,
 * not kernel time. */
int msr_search_laps(double out_us[8]);

/* The same search for query STRINGS as the reference builds them (each token repeated `weight` times,
 * src/search.py:419-422): whitespace split, token counts and dictionary lookup happen on the host inside this call —
 * the work pyserini's batch_search does in Python before handing the query to Lucene. */
int msr_search_text(msr_index* ix, const char* const* queries, int nq, int k, uint32_t flags, uint32_t* out_doc_ord,
                    float* out_score, uint32_t* out_score_u32, int32_t* out_n);

/* The host half of that call on its own: query strings -> CSR of (term id, count), out-of-vocabulary tokens dropped
 * (what pyserini's query encoding does in Python before Lucene sees the query, behind src/search.py:86-87); for callers
 * that hand the CSR to msr_hybrid_search / msr_batch_create. q_ptr (nq + 1 entries) is always filled and *n_entries is
 * set to the number of (term, count) pairs; q_term / q_w are filled when cap >= *n_entries (call with cap = 0 to size). */
int msr_encode_queries(const msr_index* ix, const char* const* queries, int nq, int64_t* q_ptr, int32_t* q_term,
                       int32_t* q_w, int64_t cap, int64_t* n_entries);

/* ---- resident batches: the same search with inputs and outputs kept in HBM (benchmark, pipelining) ---- */
int msr_batch_create(msr_index* ix, const int64_t* q_ptr, const int32_t* q_term, const int32_t* q_w, int nq,
                     int kmax, uint32_t flags, msr_batch** out);
int msr_batch_search(msr_batch* b, int k); /* enqueue on the index's stream; returns before completion */
int msr_batch_sync(msr_batch* b);
int msr_batch_fetch(msr_batch* b, uint32_t* out_doc_ord, float* out_score, uint32_t* out_score_u32,
                    int32_t* out_n); /* syncs, then copies the last search's results ([nq][k]) */
/* HIP-event durations of the last msr_batch_search on its own stream (ms): the scoring kernel and the merge. */
int msr_batch_kernel_ms(msr_batch* b, float* score_ms, float* merge_ms);
/* Sums over every msr_batch_search call since the last reset (each call records its own HIP events on the
 * index's stream), so a whole timed region can be priced without a host sync per call. */
int msr_batch_timing_reset(msr_batch* b);
int msr_batch_timing_sum(msr_batch* b, int* n_calls, float* score_ms, float* merge_ms);
/* Kept for ABI compatibility: the kernels' phase stamps were retired, so out[0..6] are zeros. out[7] = the searches of
 * this batch that took the one-workgroup-per-query walk of small indexes instead of the staged launches.
 * Returns MSR_OK (MSR_E_INVAL for a null batch or output). */
int msr_batch_debug_stamps(msr_batch* b, unsigned long long out[8]);
/* Algorithmic bytes of one search of this batch, SURVEY.md §8d:
 * sum over queries of  sum_t df(t)*(4+2) + |q|*12 + k*8  (df restricted to this handle's shard). */
int msr_batch_algo_bytes(const msr_batch* b, int k, uint64_t* bytes, uint64_t* postings);
/* The work one search of this batch does, for the roofline of the scoring kernel (no reference counterpart):
 * out = {postings walked through inverted lists (one LDS add each), postings scored out of the dense head (half a
 * v_dot2_u32_u16 each), (tile, query) workgroups, LDS bytes written to initialise the accumulator tiles, LDS bytes the
 * selection reads back (two passes), kept query entries}. */
int msr_batch_work(const msr_batch* b, uint64_t out[6]);
void msr_batch_destroy(msr_batch* b);

/* ---- multi-GPU exchange (doc-range shards, one RCCL all-gather of per-shard top-k) ----
 * No counterpart in the reference (it never shards the sparse index, src/search.py:216,273). */
#define MSR_COMM_ID_BYTES 128
int msr_comm_unique_id(char id[MSR_COMM_ID_BYTES]);
int msr_comm_init(msr_index* ix, int n_ranks, int rank, const char id[MSR_COMM_ID_BYTES]);
/* local search + all-gather + merge; afterwards msr_batch_fetch returns the GLOBAL top-k on every rank. */
int msr_batch_search_sharded(msr_batch* b, int k);
int msr_comm_destroy(msr_index* ix);
/* What the communicator of `ix` reports about itself (ncclCommCount / ncclCommUserRank / ncclCommCuDevice). */
int msr_comm_info(const msr_index* ix, int* n_ranks, int* rank, int* device);
/* One line of text for logs and the benchmark record: HIP runtime version, RCCL version and the path of the librccl
 * the process actually resolved (dladdr). */
int msr_runtime_info(char* buf, int cap);
/* hipDeviceSynchronize on `device` (the benchmark's device-wide fence, independent of any torch state). */
int msr_device_sync(int device);
/* Bandwidth of a device-to-device copy of `bytes` (read + write bytes / time, GB/s): the measured HBM figure quoted
 * beside the vendor peak in the benchmark record. */
int msr_device_copy_gbs(int device, uint64_t bytes, int reps, double* gbs);
/* Measured peaks of the pipes the scoring kernel's useful work runs on, at its launch shape (512 threads, four
 * workgroups per CU): out = {ds_add_u32 lane operations / s, v_dot2_u32_u16 lane operations / s, LDS bytes / s at one
 * 16-byte write per two 16-byte reads, CUs}. Takes a few milliseconds. */
int msr_device_peak_rates(int device, double out[4]);

/* Term-range shards (the north star's partition; exact protocol of DESIGN.md §6): the batch holds only the query terms
 * of term range `shard` of `n_shards` (ranges are contiguous in term id and balanced by postings). Search = dump the
 * partial accumulators, ncclReduceScatter(sum) them into doc ranges, select, all-gather, merge. The handle must hold
 * every doc tile (msr_index_open) and the communicator's rank / size must equal shard / n_shards. */
int msr_batch_create_termshard(msr_index* ix, const int64_t* q_ptr, const int32_t* q_term, const int32_t* q_w, int nq,
                               int kmax, uint32_t flags, int shard, int n_shards, msr_batch** out);
int msr_batch_search_termshard(msr_batch* b, int k);
/* The same protocol for `n_shards` logical term shards played on one GPU (sums in place instead of RCCL). */
int msr_search_termshard_emulated(msr_index* ix, const int64_t* q_ptr, const int32_t* q_term, const int32_t* q_w, int nq,
                                  int k, uint32_t flags, int n_shards, uint32_t* out_doc_ord, float* out_score,
                                  uint32_t* out_score_u32, int32_t* out_n);
/* ... and with one handle per logical shard, shards[g] opened by msr_index_open_termshard(path, dev, g, n_shards) on
 * the same device: every shard scores out of its own partial residency. */
int msr_search_termshard_emulated_handles(msr_index* const* shards, int n_shards, const int64_t* q_ptr,
                                          const int32_t* q_term, const int32_t* q_w, int nq, int k, uint32_t flags,
                                          uint32_t* out_doc_ord, float* out_score, uint32_t* out_score_u32, int32_t* out_n);

/* Merge `n_lists` per-shard result lists (each [nq][k] as written by msr_batch_fetch) on the device of `ix`
 * with the same tie rule; used by the host-side exchange (torch.distributed all_gather) and by tests. */
int msr_merge_lists(msr_index* ix, int n_lists, int nq, int k, const uint32_t* doc_ord, const uint32_t* score_u32,
                    const int32_t* n, uint32_t* out_doc_ord, float* out_score, uint32_t* out_score_u32,
                    int32_t* out_n);

/* ---- dense flat inner-product search (hybrid path): replaces tevatron FaissFlatSearcher / faiss IndexFlatIP with
 * fp16 storage (src/search.py:232-237,254-270; call site search_queries src/search.py:55-63).
 * p_fp16 / q_fp16 are row-major IEEE fp16 matrices ([n][h] / [nq][h], h a multiple of 32); scores are f32-accumulated
 * on MFMA. Outputs [nq][k]: row indices (0xFFFFFFFF padding), order-preserving u32 keys of the f32 scores
 * (key = bits ^ 0x80000000 for non-negative, ~bits for negative floats; 0 = padding) and the hit count. */
typedef struct msr_dense msr_dense;
int msr_dense_open(const uint16_t* p_fp16, uint64_t n, uint32_t h, int device, msr_dense** out);
int msr_dense_search(msr_dense* dx, const uint16_t* q_fp16, int nq, int k, uint32_t* out_idx, uint32_t* out_key,
                     int32_t* out_n, float* gemm_ms, float* select_ms);
/* ---- f32 flat search: tevatron's FaissFlatSearcher as the reference runs it without --use_gpu (a plain f32 faiss
 * IndexFlatIP on the CPU: src/arguments.py:63, src/search.py:232-237; the dense-only recipe scripts/search_dense.sh).
 * p / q are row-major f32 matrices ([n][h] / [nq][h], any h >= 1, inputs expected finite). Numeric contract: every
 * score is the k-ordered fmaf chain
 *     s = fmaf(q[h-1], p[h-1], ... fmaf(q[1], p[1], fmaf(q[0], p[0], +0.0f)))
 * bit for bit (v_mfma_f32_32x32x2_f32, one accumulator per score, no split-K, subnormals kept), so a score does not
 * depend on the batch it was searched in. Outputs, key map, padding and tie rule (lower ROW wins) are those of
 * msr_dense_search; 1 <= k <= MSR_KMAX. A handle holds one precision: msr_dense_search on an f32 handle,
 * msr_dense_search_f32 on an fp16 handle, msr_hybrid_search with an f32 handle and msr_hybrid_search_f32 with an fp16
 * handle fail with MSR_E_INVAL.
 * msr_dense_close and msr_dense_stats serve both kinds. */
int msr_dense_open_f32(const float* p, uint64_t n, uint32_t h, int device, msr_dense** out);
int msr_dense_search_f32(msr_dense* dx, const float* q, int nq, int k, uint32_t* out_idx, uint32_t* out_key,
                         int32_t* out_n, float* gemm_ms, float* select_ms);
/* ---- exact ranks of listed rows on the dense route: "where does this row stand for this query", at any depth. The
 * dense counterpart of msr_rank_docs: a flat search stops at k <= MSR_KMAX, so a judged row below that is missing from
 * its lists and MedR / MeanR / MRR / Recall@k beyond it cannot be computed from a run. NO counterpart call in the
 * reference, tevatron or faiss.
 * q is [nq][h] row-major in the handle's precision: q_is_f32 = 1 for f32 rows and a handle from msr_dense_open_f32,
 * q_is_f32 = 0 for fp16 rows and a handle from msr_dense_open; a mismatch is MSR_E_INVAL. Inputs are expected finite.
 * The listed rows (targets) are CSR: query i owns entries [t_ptr[i], t_ptr[i+1]) of t_row (dense ROW indices; at most
 * MSR_DENSE_RANK_MAX_TARGETS per query, duplicates allowed, none is fine). Both outputs are indexed like t_row. With
 * key(d) the u32 key of the score this handle's GEMM gives row d for query i (the key map and the kernels of
 * msr_dense_search / msr_dense_search_f32):
 *     out_key  = key(t)
 *     out_rank = 0 when t == self_row[i],
 *                else 1 + #{ d in [0, n), d != self_row[i] : key(d) > key(t) or (key(d) == key(t) and d < t) }
 * Every row is a hit (a flat index returns any score: there is no "score 0 = not ranked" rule), the order is by KEY (so
 * -0 ranks below +0 exactly as the search orders them) and a score tie goes to the lower ROW, as in msr_dense_search.
 * self_row (nullable; a negative entry = none) names the row remove_query drops (src/search.py:72-74).
 * Link to the search: with self_row NULL and any 1 <= k <= MSR_KMAX, t is in row i of the search at k exactly when
 * rank <= k, at column rank - 1 with the same key. On an f32 handle this holds whatever batches the two calls were made
 * with (every key is the k-ordered fmaf chain). On an fp16 handle it holds when both calls get the same query matrix
 * (the same nq, hence the same passes and the same GEMM instance; the two fp16 GEMM instances need not round alike).
 * ms (nullable) = HIP-event times summed over the passes: {query upload + GEMM, the count kernel}.
 * Argument errors are reported before any device work: MSR_E_INVAL for a null dx / t_ptr, a null q with nq > 0, a null
 * t_row / output with entries to write, nq < 0, a t_ptr that does not start at 0 or decreases, the precision mismatch;
 * MSR_E_RANGE for a row or a self_row entry >= n and for more than MSR_DENSE_RANK_MAX_TARGETS targets in one query.
 * nq == 0 or no target at all returns MSR_OK without a launch and with ms = {0, 0}. The scratch stays with the handle
 * like the search's (msr_dense_stats). */
#define MSR_DENSE_RANK_MAX_TARGETS 64 /* listed rows per query */
int msr_dense_rank_rows(msr_dense* dx, const void* q, int q_is_f32, int nq, const int64_t* t_ptr, const uint32_t* t_row,
                        const int32_t* self_row, uint32_t* out_rank, uint32_t* out_key, float ms[2]);
/* Deep lists on the dense route: the dense search for 1 <= k <= MSR_DEEP_KMAX (else MSR_E_RANGE). Serves both handle
 * kinds: q is [nq][h] in the handle's precision and q_is_f32 must match the handle (else MSR_E_INVAL), as in
 * msr_dense_rank_rows. The passes and the GEMM are those of msr_dense_search / msr_dense_search_f32, so on an fp16 handle
 * the same query matrix gives the same keys; the exact top-k of every key row is then taken by deep_select_rows instead
 * of the tile selection and merge. Outputs ([nq][k] row indices and keys, out_n), the key map, the padding (0xFFFFFFFF /
 * 0) and the tie rule (lower ROW) are those of msr_dense_search; every row is a hit, so out_n[i] = min(k, n).
 * IDENTITIES: for k <= MSR_KMAX the outputs are bit-equal to the search at that k on the same query matrix; for any k,
 * columns [0, min(k, 1024)) equal the search at k = 1024; the row at column c of query i has rank c + 1 from
 * msr_dense_rank_rows on the same query matrix with self_row NULL.
 * ms (nullable) = HIP-event times summed over the passes: {query upload + GEMM, the deep selection}. Argument errors
 * are reported before any device work: MSR_E_INVAL (a null dx / output, a null q with nq > 0, nq < 0, the precision
 * mismatch), then MSR_E_RANGE (k). nq == 0 returns MSR_OK without a launch. The scratch stays with the handle and only
 * grows (msr_dense_stats shows no allocation on a repeated call of one shape). */
int msr_dense_search_deep(msr_dense* dx, const void* q, int q_is_f32, int nq, int k, uint32_t* out_idx,
                          uint32_t* out_key, int32_t* out_n, float ms[2]);
/* Filtered search on the dense route: msr_dense_search / msr_dense_search_f32 among the rows of each query's set. The doc
 * sets are those of msr_search_filtered with n = the number of rows and bits over ROW indices. q is [nq][h] in the handle's
 * precision and q_is_f32 must match the handle (else MSR_E_INVAL), as in msr_dense_search_deep. Every row of the set is a
 * hit (a flat index returns any score), so out_n[i] = min(k, |set|); order by key descending, ties to the lower ROW;
 * outputs, key map and padding (0xFFFFFFFF / 0) are those of msr_dense_search; 1 <= k <= MSR_KMAX. The passes and the
 * GEMM are the search's, so the same query matrix gives the same keys; select_tiles_filtered masks the keys on their way
 * into LDS and the search's merge follows.
 * IDENTITIES: a full set, or q_set = -1, is bit-equal to the search at that k on the same query matrix; for any set the
 * list equals msr_dense_search_deep at a k that covers every row, with the non-members struck out, cut to k; a set and
 * its complement partition the rows.
 * ms (nullable) = HIP-event times summed over the passes: {query upload + GEMM, selection + merge}. Argument errors are
 * reported before any device work, in this order: MSR_E_INVAL (a null dx / output, a null q with nq > 0, nq < 0,
 * n_sets < 0, a null set_bits with n_sets > 0, a null q_set with n_sets > 1, the precision mismatch); MSR_E_RANGE (k,
 * n_sets > MSR_FILTER_MAX_SETS, a q_set entry outside [-1, n_sets)); MSR_E_NODEVICE. nq == 0 returns MSR_OK without a
 * launch. The scratch stays with the handle and only grows. */
int msr_dense_search_filtered(msr_dense* dx, const void* q, int q_is_f32, int nq, int k, const uint32_t* set_bits,
                              int n_sets, const int32_t* q_set, uint32_t* out_idx, uint32_t* out_key, int32_t* out_n,
                              float ms[2]);
void msr_dense_close(msr_dense* dx);
/* Bookkeeping of a dense handle: out = {hipMalloc calls made for its scratch so far, scratch bytes it holds, rows, dim}.
 * The scratch of msr_dense_search / msr_hybrid_search stays with the handle and is only ever grown, so repeated calls of
 * one shape allocate nothing (the reference searches in batches of 2, scripts/search.sh:29). */
int msr_dense_stats(const msr_dense* dx, uint64_t out[4]);
/* Host helper for the two calls above: n f32 values -> IEEE fp16, round to nearest even (what numpy's astype(float16)
 * and the reference's .half() produce: src/search.py:257; bit-identical for every non-NaN input — a NaN comes out
 * quiet, numpy keeps its payload), on `threads` host threads (<= 0: all). The reference hands
 * its query matrix over in f32 (src/search.py:342-343); converting 25 010 x 4 096 values in numpy takes longer than
 * the whole GPU search. */
int msr_f32_to_f16(const float* src, uint16_t* dst, uint64_t n, int threads);

/* ---- hybrid search on the GPU: sparse top-`depth` + dense top-`depth` + the reference's min-max fusion
 * (fuse, src/hybrid.py:32-53, weights [alpha, 1-alpha] src/search.py:459) + top-k, without leaving HBM in between.
 * row2ord[r] = sparse doc ordinal of dense row r; self_ord[q] (nullable) = ordinal removed from query q's lists
 * (remove_query, src/search.py:72-74) or -1. row2ord must be a permutation of the ordinals. depth, k <= MSR_KMAX.
 * The GEMM runs on the passage rows permuted into ordinal order (built once per mapping, kept on the dense handle), so a
 * query's row of dense scores lines up with the sparse accumulator tiles, and no list ever leaves HBM:
 *   - one tile (n_docs <= 8192), k <= 64: ONE kernel per query does sparse scoring, both depth selections, fusion and
 *     top-k (hybrid_tiles); ms = {that kernel, dense GEMM, 0, 0};
 *   - otherwise (the reference's own hybrid run: 25 010 caption docs = 4 tiles, scripts/search.sh): one workgroup per
 *     (tile, query) scores the tile and emits its quota of candidates for both depth lists, one workgroup per query
 *     finds both depth-th bests among them, fuses and ranks; a query whose depth list a tile's quota did not cover
 *     (verified per query) is repeated with every tile's own top-depth, so the result is exact whatever the quota;
 *     ms = {candidate kernel, dense GEMM, 0, fusion kernel};
 *   - tile sizes other than 4096 / 8192 docs, shard handles, MSR_NO_FUSED_HYBRID: the list-based path (score_tiles at
 *     k = depth, select_tiles over the score matrix, fuse_tiles, merges); ms = {sparse, dense GEMM, dense select, fusion}.
 * Tie rule of the DENSE depth list (two passages with bit-equal scores at the depth boundary — duplicated captions do
 * that): the first two paths keep the lower doc ORDINAL, the list-based path and msr_dense_search the lower ROW, as a
 * flat index does. Everything else (sparse ties, fused-score ties: lower ordinal) is the same on every path.
 * FUSION CONTRACT. Every path computes the fused score by this f32 operation sequence, bit for bit:
 *     w_d = (float)alpha, w_s = 1.0f - w_d;
 *     per side: max / min = the best and the last score of the UNFILTERED depth list (self_ord still in it) — sparse:
 *         (float)u32, dense: -0 canonicalised to +0, an empty list: 0, 0 — and inv = 1.0f / fmaxf(max - min, 1e-9f);
 *     t(x) = 1.0f when x is the list's maximum and max > min (the sparse comparison is on the exact u32 score, not on
 *         its f32 image), else t(x) = (x - min) * inv: one rounded subtraction, one rounded multiplication;
 *     f = +0.0f;  f = fmaf(w_d, t_d, f) if the dense list holds the doc;  f = fmaf(w_s, t_s, f) if the sparse list does.
 * Members are the union of the two lists minus self_ord, ordered by the fused key descending, lower ordinal first; the
 * first k are returned, out_n = min(k, members), padding 0xFFFFFFFF / 0.f. So the same depth lists give the same
 * ordinals and score bits on every path; only the dense tie rule above can make the lists differ. alpha outside [0, 1]
 * is not refused (one weight is negative, fused scores may be). tests/fusion_ref.py restates the sequence in numpy. */
int msr_hybrid_search(msr_index* ix, msr_dense* dx, const int64_t* q_ptr, const int32_t* q_term, const int32_t* q_w,
                      const uint16_t* q_fp16, int nq, int depth, int k, float alpha, uint32_t flags,
                      const uint32_t* row2ord, const int32_t* self_ord, uint32_t* out_ord, float* out_score, int32_t* out_n,
                      float ms[4]);
/* ---- f32 hybrid search: msr_hybrid_search with the dense side of the reference's default run (an f32 IndexFlatIP,
 * no --use_gpu: src/arguments.py:63, src/search.py:232-237,254-270). The contract is msr_hybrid_search's — the same three
 * paths chosen by the same rules, the same ms layout, the same dense tie rule per path — except that:
 *   - dx comes from msr_dense_open_f32 (an fp16 handle: MSR_E_INVAL; an f32 handle given to msr_hybrid_search: likewise);
 *   - q is [nq][h] row-major f32, any h >= 1;
 *   - every dense score is the k-ordered fmaf chain of msr_dense_search_f32, so it has the same bits as that call on the
 *     same rows (the two fused paths run the same f32 GEMM on the ordinal-ordered rows, a second n_pad x hp x 4-byte
 *     copy on the device, built once per mapping and freed by msr_dense_close). */
int msr_hybrid_search_f32(msr_index* ix, msr_dense* dx, const int64_t* q_ptr, const int32_t* q_term, const int32_t* q_w,
                          const float* q, int nq, int depth, int k, float alpha, uint32_t flags, const uint32_t* row2ord,
                          const int32_t* self_ord, uint32_t* out_ord, float* out_score, int32_t* out_n, float ms[4]);
/* ---- the whole fused union and both depth lists from one call: what the reference's hybrid run writes per query — the
 * sparse top-`depth` list, the dense top-`depth` list and fuse() of the two, which keeps EVERY doc of either list
 * (src/search.py:455-461, src/hybrid.py:32-53) — plus, per fused doc, the list(s) it came from (fuse_statistic,
 * src/hybrid.py:56-90). Inputs mean what they mean for msr_hybrid_search / msr_hybrid_search_f32; q is [nq][h] fp16
 * (q_is_f32 = 0, dx from msr_dense_open) or f32 (q_is_f32 = 1, dx from msr_dense_open_f32), a mismatch is MSR_E_INVAL.
 * 1 <= depth <= MSR_KMAX; there is no k. Every per-member output is row-major [nq][2 * depth]; row i holds out_n[i]
 * members = the union of query i's two depth lists minus self_ord[i], by fused score descending (ties: lower ordinal);
 * a member whose fused score is 0 (the depth-th doc of one list that is not in the other) IS a member. Padding:
 * 0xFFFFFFFF / 0.f as msr_hybrid_search pads, 0 in the optional arrays.
 *   out_score       the f32 fused score of msr_hybrid_search[_f32] (the FUSION CONTRACT above): the first
 *                   min(k, out_n[i]) entries of a row have the ordinals and the score bits those calls return for that k;
 *   out_src         bit 0: in the dense depth list, bit 1: in the sparse depth list (1 / 2 / 3 = fuse_statistic's
 *                   'dense' / 'sparse' / 'fuse' with runs ordered [dense, sparse], src/search.py:459);
 *   out_sparse_u32  the exact sparse score where bit 1 is set, else 0;
 *   out_dense       the f32 dense score where bit 0 is set, else 0 (f32 handle: the bits of msr_dense_search_f32);
 *   out_range[i]    {dense max, dense min, sparse max, sparse min}: the best and the depth-th (or last) score of each
 *                   UNFILTERED list, which the fusion normalises with and get_run_dict stores (src/search.py:76-81);
 *                   {0, 0} for an empty list. Not recoverable from the members when self_ord[i] was the best or the last.
 * The four optional outputs may be NULL: such an array is neither computed into host memory nor downloaded.
 * ms = {candidate kernel, dense GEMM, 0, fusion kernel}. Supported handles: those of msr_hybrid_search's candidate path
 * (whole index, 4096- or 8192-doc tiles, fp16: h % 8 == 0), a single-tile index included; any other handle is refused
 * with MSR_E_INVAL (no list-based union; MSR_NO_FUSED_HYBRID is not read). Dense ties at the depth boundary: lower
 * ordinal. Scratch stays on the dense handle and only grows. */
#define MSR_UNION_MAX (2 * MSR_KMAX) /* most docs a fused union can hold */
int msr_hybrid_search_union(msr_index* ix, msr_dense* dx, const int64_t* q_ptr, const int32_t* q_term, const int32_t* q_w,
                            const void* q, int q_is_f32, int nq, int depth, float alpha, uint32_t flags,
                            const uint32_t* row2ord, const int32_t* self_ord, uint32_t* out_ord, float* out_score,
                            int32_t* out_n, uint8_t* out_src, uint32_t* out_sparse_u32, float* out_dense, float* out_range,
                            float ms[4]);
/* ---- alpha sweep: ONE hybrid scoring fused at many alphas. alpha is the one number the reference's hybrid run is tuned
 * by (--alpha, weights = [alpha, 1 - alpha], src/search.py:459, fuse(), src/hybrid.py:32-53), and nothing before the last
 * two fmafs of the FUSION CONTRACT depends on it: the depth lists, their members, their extremes and every t_d / t_s are
 * the same at every alpha. This call runs the union pass of msr_hybrid_search_union once (sparse scores, GEMM, both
 * depth selections, the union), keeps its outputs on the device and re-fuses and re-ranks them per alpha (fuse_sweep),
 * where a sweep over msr_hybrid_search[_f32] pays the whole scoring once per alpha.
 * Inputs mean what they mean for msr_hybrid_search_union; q_is_f32 must match the handle. alphas: n_alphas floats,
 * duplicates allowed, values outside [0, 1] not refused (as in msr_hybrid_search), a non-finite one is MSR_E_INVAL.
 * 1 <= depth <= MSR_KMAX, 1 <= k <= 2 * depth, 1 <= n_alphas <= MSR_SWEEP_MAX_ALPHAS.
 * Outputs: out_ord / out_score row-major [n_alphas][nq][k], out_n [n_alphas][nq]; padding 0xFFFFFFFF / 0.f.
 * CONTRACT / IDENTITIES, all bit for bit:
 *   - slice a = the first k columns of msr_hybrid_search_union at alpha = alphas[a]: ordinals, score bits,
 *     out_n = min(k, that call's out_n);
 *   - hence, for k <= MSR_KMAX, slice a = msr_hybrid_search[_f32] at that alpha, depth and k, on whichever of the two
 *     candidate / fused paths that call takes (both use the lower-ordinal dense tie rule);
 *   - slice a = tests/fusion_ref.topk(fuse(S, D, depth, alphas[a], self_ord), k);
 *   - a slice depends neither on which other alphas are in the call nor on their order.
 * t_s = 1 is decided on the exact u32 sparse maximum of the unfiltered list, which the union pass hands to the sweep
 * beside out_range's f32 images (a member can share the maximum's image without being the maximum).
 * ms = {candidate kernel, dense GEMM, 0, the union pass's fusion kernel, the sweep kernel(s) summed, number of alpha
 * groups launched}: the alphas go in groups whose [group][nq][k] lists fit 256 MiB of device staging (at least one alpha per
 * group), each group is downloaded before the next is launched.
 * Supported handles: msr_hybrid_search_union's (whole index, 4096- or 8192-doc tiles, a single-tile index included,
 * fp16: h % 8 == 0); any other handle is MSR_E_INVAL. The tile quota (MSR_HYBRID_QUOTA) and the second round only affect
 * the pass before the sweep. Scratch stays on the dense handle and only grows: a repeated call of one shape allocates
 * nothing (msr_dense_stats).
 * Argument errors, before any device work, in this order: MSR_E_INVAL (null ix / dx / q_ptr / alphas / row2ord / outputs, a
 * null q with nq > 0, nq < 0, the precision mismatch, row counts that differ, an unsupported or shard handle, a
 * non-finite alpha); MSR_E_RANGE (depth, k, n_alphas); MSR_E_NODEVICE. nq == 0 returns MSR_OK without a launch. */
#define MSR_SWEEP_MAX_ALPHAS 64
int msr_hybrid_sweep(msr_index* ix, msr_dense* dx, const int64_t* q_ptr, const int32_t* q_term, const int32_t* q_w,
                     const void* q, int q_is_f32, int nq, int depth, int k, const float* alphas, int n_alphas,
                     uint32_t flags, const uint32_t* row2ord, const int32_t* self_ord,
                     uint32_t* out_ord, float* out_score, int32_t* out_n, float ms[6]);

/* ---- deep hybrid search: the fused union of two depth lists of up to MSR_DEEP_KMAX docs each, at one or many alphas. The
 * reference treats --depth as a free integer and writes the whole fused union (src/arguments.py:59, src/search.py:455-461,
 * src/hybrid.py:32-53); the candidate paths above hold at most MSR_KMAX docs per depth list. This call never builds
 * candidate lists: per pass of queries it writes the exact u32 sparse scores of every doc as one row (the accumulator dump
 * of msr_search_deep) and the dense keys of every doc as another (the hybrid GEMM on the ordinal-ordered rows, key map of
 * msr_dense_search), takes both depth lists with deep_select_rows at k = depth, and fuses the two ROWS elementwise
 * (fuse_rows): a doc is in a depth list exactly when its (key, ordinal) composite is at or above the list's last one, so
 * the lists' first key, last key and last ordinal are all that fusion needs. The fused top-k is one more deep_select_rows
 * over the row of fused keys. Scoring, the GEMM and both depth selections run once per pass, however many alphas.
 * Inputs mean what they mean for msr_hybrid_sweep; q_is_f32 must match the handle. 1 <= depth <= MSR_DEEP_KMAX,
 * 1 <= k <= min(2 * depth, MSR_DEEP_KMAX), 1 <= n_alphas <= MSR_SWEEP_MAX_ALPHAS.
 * Outputs: out_ord / out_score row-major [n_alphas][nq][k] and out_n [n_alphas][nq] (padding 0xFFFFFFFF / 0.f);
 *   out_members[nq]  the size of the union minus self_ord: the same at every alpha, and larger than out_n where k cut the
 *                    union (possible only when 2 * depth > MSR_DEEP_KMAX or k < 2 * depth);
 *   out_src          [n_alphas][nq][k], NULLABLE: bit 0 dense list, bit 1 sparse list, 0 padding;
 *   out_sparse_ord / out_sparse_u32 [nq][depth], out_sparse_n [nq]: the sparse depth list, each NULLABLE;
 *   out_dense_ord / out_dense [nq][depth] (f32 scores), out_dense_n [nq]: the dense depth list, each NULLABLE;
 *   out_range        [nq][4] as in msr_hybrid_search_union, NULLABLE.
 * Dense ties at the depth boundary go to the lower ordinal, as on both fused paths. A member whose fused score is +0
 * IS a member. IDENTITIES, all bit for bit:
 *   (a) depth <= MSR_KMAX, on a handle msr_hybrid_search_union serves: slice a at k = 2 * depth equals that call at
 *       alphas[a] (ordinals, score bits, out_n, out_src, out_range), and both depth lists equal its members with the
 *       matching source bit. On an f32 handle every key is the k-ordered fmaf chain. On an fp16 handle both calls take the
 *       SAME GEMM instance whatever the batch (the hybrid paths choose it by h and the doc count alone, never by nq), so
 *       the identity needs the same query rows and nothing of the batch's size;
 *   (b) any depth: the fused outputs equal tests/fusion_ref.topk(fuse(S, D, depth, alpha, self_ord), k), the sparse list
 *       equals msr_search_deep at k = depth, the dense list equals the d_lists of fusion_ref.fuse (out_dense: their f32
 *       scores);
 *   (c) a slice depends neither on the other alphas of the call nor on their order.
 * One caveat to (a) and (b): the dense keys are ranked as the GEMM writes them, and its key map puts a dense score of -0
 * directly below +0, where the candidate paths and fusion_ref rank x + 0.0f. A GEMM accumulator starts at +0, so -0 comes
 * out only when every product of a row is a negative underflow; for such a doc the dense depth list and the order inside
 * the zero tie class can differ from those calls. fuse_rows reads the score as +0 (dense + 0.0f), as they do.
 * Passes: the largest of the three row buffers of a pass (sparse scores and fused keys [queries][n_tiles * tile_docs],
 * dense keys [queries][docs rounded up to 256]) holds at most 256 MiB, with the queries of a pass rounded down to whole
 * row blocks of the hybrid GEMM (256 on fp16 handles, 128 on f32 ones) and never fewer than one block.
 * Handles: whole-index handles only (a doc-range or term-range shard handle: MSR_E_INVAL). ALL five tile sizes are
 * served: neither producer depends on the candidate kernels, so no tile size is refused. Scratch stays on the dense
 * handle and only grows: a repeated call of one shape allocates nothing (msr_dense_stats).
 * ms = {sparse scoring, query upload + GEMM, the two depth selections, fuse_rows summed over the alphas, the fused
 * selections summed, number of passes}.
 * Argument errors, before any device work, in this order: MSR_E_INVAL (null ix / dx / q_ptr / alphas / row2ord / out_ord /
 * out_score / out_n / out_members, a null q with nq > 0, nq < 0, the precision mismatch, row counts that differ, a shard
 * handle, a non-finite alpha); MSR_E_RANGE (depth, k, n_alphas); MSR_E_NODEVICE. nq == 0 returns MSR_OK without a launch. */
int msr_hybrid_deep(msr_index* ix, msr_dense* dx, const int64_t* q_ptr, const int32_t* q_term, const int32_t* q_w,
                    const void* q, int q_is_f32, int nq, int depth, int k, const float* alphas, int n_alphas,
                    uint32_t flags, const uint32_t* row2ord, const int32_t* self_ord,
                    uint32_t* out_ord, float* out_score, int32_t* out_n, uint32_t* out_members, /* fused */
                    uint8_t* out_src,
                    uint32_t* out_sparse_ord, uint32_t* out_sparse_u32, int32_t* out_sparse_n, /* depth lists, nullable */
                    uint32_t* out_dense_ord, float* out_dense, int32_t* out_dense_n,
                    float* out_range, float ms[6]);

/* ---- filtered deep hybrid search: msr_hybrid_deep among the docs of each query's set. The doc sets are exactly those of
 * msr_search_filtered: set_bits is [n_sets][(n_docs + 31) / 32], bitmaps over doc ORDINALS (bits at or above n_docs are
 * ignored); q_set[i] in [-1, n_sets), -1 = unfiltered; q_set may be NULL when n_sets is 0 (nothing filtered) or 1 (every
 * query uses set 0); at most MSR_FILTER_MAX_SETS sets. One bitmap serves both sides: the hybrid GEMM runs on the
 * ordinal-ordered rows. Every other input and every output is msr_hybrid_deep's.
 * CONTRACT, for query i with set M (all docs when unfiltered): the sparse depth list is the exact top-depth of
 * {d in M : s(d) > 0}; the dense depth list is the exact top-depth of M (every member is a hit, ties go to the lower
 * ordinal); the extremes and out_range are those of these two lists, with self_ord still in them when it is a member;
 * everything after that is the FUSION CONTRACT and msr_hybrid_deep's contract word for word (members, out_members,
 * out_src, padding, the k cut, the -0 caveat). A self_ord outside M changes nothing. The result is what an index that
 * holds only M's docs would give.
 * How: both score rows of msr_hybrid_deep are masked by the set (score_dump_filtered writes a masked sparse row,
 * mask_key_rows zeroes the dense keys of the non-members) and a key of 0 is "not a member" to every step after that, so
 * both depth selections, fuse_rows, the fused selection and the source gather run unchanged. A pass without a filtered
 * query issues exactly msr_hybrid_deep's launches.
 * IDENTITIES, all bit for bit:
 *   (a) a full set, q_set[i] = -1 or n_sets = 0 gives row i of msr_hybrid_deep on the same inputs in every output, per
 *       query in a batch that mixes filtered and unfiltered queries;
 *   (b) for any set, row i equals tests/fusion_ref.fuse run on the sub-corpus of M's columns (S and D restricted to M,
 *       self_ord moved to its position in M or to -1, ordinals mapped back): tests/hybrid_filter_ref.py;
 *   (c) the sparse depth list equals msr_search_filtered at k = depth for depth <= MSR_KMAX, and msr_search_deep with the
 *       non-members struck out for larger depths;
 *   (d) an empty set, or a set with no doc at all, gives out_n = 0, out_members = 0, out_range = {0, 0, 0, 0}, empty
 *       depth lists and padding everywhere;
 *   (e) a slice depends neither on the other alphas nor on the sets of the other queries.
 * Handles, passes and scratch are msr_hybrid_deep's (whole-index handles, all five tile sizes, fp16 and f32 dense handles;
 * the scratch stays on the dense handle and only grows); the set image travels with the call's own upload.
 * ms = msr_hybrid_deep's six slots (the filtered dump is timed in slot 0), then ms[6] = mask_key_rows summed over the
 * passes, 0 when no query is filtered.
 * Argument errors, before any device work, in this order: MSR_E_INVAL (msr_hybrid_deep's, then n_sets < 0, a null
 * set_bits with n_sets > 0, a null q_set with n_sets > 1); MSR_E_RANGE (depth, k, n_alphas, then n_sets >
 * MSR_FILTER_MAX_SETS and a q_set entry outside [-1, n_sets)); MSR_E_NODEVICE. nq == 0 returns MSR_OK without a launch. */
int msr_hybrid_deep_filtered(msr_index* ix, msr_dense* dx, const int64_t* q_ptr, const int32_t* q_term, const int32_t* q_w,
                             const void* q, int q_is_f32, int nq, int depth, int k, const float* alphas, int n_alphas,
                             uint32_t flags, const uint32_t* row2ord, const int32_t* self_ord,
                             const uint32_t* set_bits, int n_sets, const int32_t* q_set,
                             uint32_t* out_ord, float* out_score, int32_t* out_n, uint32_t* out_members, /* fused */
                             uint8_t* out_src,
                             uint32_t* out_sparse_ord, uint32_t* out_sparse_u32, int32_t* out_sparse_n, /* depth lists, nullable */
                             uint32_t* out_dense_ord, float* out_dense, int32_t* out_dense_n,
                             float* out_range, float ms[7]);

/* ---- encode-side sparsifier: log(1 + relu(logit)) -> top-k -> rint(x * 100) (src/model.py:104, src/encode.py:69-75).
 * logits: row-major [rows][vocab], f32 (is_f16 = 0) or IEEE fp16 (is_f16 = 1). fp16_math = 1 rounds 1 + relu and the
 * log to half like a model running in fp16. Outputs [rows][k]: vocabulary ids (ties: lower id first), the selected
 * values v and the integer weights rint(v * 100). */
int msr_sparsify(const void* logits, int is_f16, int fp16_math, int rows, uint32_t vocab, int k, int device,
                 uint32_t* out_idx, float* out_val, int32_t* out_weight);

/* ---- synthetic encode step (SURVEY.md §8d generator; stands in for src/encode.py when no MLLM is present) ----
 * Fills a doc-major CSR of n vectors with `nnz` distinct terms each, drawn without replacement from
 * p(r) ~ r^-zipf_s over n_terms, weights max(1, rint(100*ln(1+x))), x ~ LogNormal(0.5, 0.6), clipped to [1,400].
 * ptr has n+1 entries; term/weight have n*nnz. Deterministic in (seed, row) regardless of threads. */
int msr_synth_vectors(uint64_t n, uint32_t nnz, uint32_t n_terms, double zipf_s, uint64_t seed, int threads,
                      uint64_t* ptr, uint32_t* term, uint32_t* weight);

const char* msr_last_error(void);
const char* msr_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MSR_H */
