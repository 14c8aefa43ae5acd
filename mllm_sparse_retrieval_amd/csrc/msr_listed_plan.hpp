// Host side of the listed-docs calls msr_rank_docs, msr_explain_docs and msr_doc_vectors (plain C++, no HIP; included by
// msr_rank.hpp, msr_explain.hpp and msr_doc_vectors.hpp): the tables their kernels read, built from the caller's arrays
// after the argument checks and, for the two calls that take queries, the search path's query normalisation have passed
// (every term id of a counting entry is below n_terms, every ordinal below n_docs, at most MSR_RANK_MAX_TARGETS /
// MSR_EXPLAIN_MAX_TARGETS listed docs per query, fewer than 2^32 output slots).
#pragma once

#include <algorithm>
#include <utility>

#include "msr_internal.h"

namespace msr {

// A listed doc of query q: `slot` is where its result goes (rank: the entry, or n_entries + q for the self doc; explain:
// the first output slot of its row), local = ordinal - tile * tile_docs.
struct ListedItem {
    uint32_t tile, q, slot, local;
};

// The two tables a kernel over listed docs reads. The docs are ordered by (tile, query), keeping the given order inside a
// pair: `items` gets one row {slot, local} per doc, `pairs` one row {query, tile, first item, items} per pair, tile-major
// so that neighbouring workgroups share the tile.
inline void group_pairs(std::vector<ListedItem>& its, std::vector<uint32_t>& pairs, std::vector<uint32_t>& items) {
    std::stable_sort(its.begin(), its.end(),
                     [](const ListedItem& x, const ListedItem& y) { return x.tile != y.tile ? x.tile < y.tile : x.q < y.q; });
    pairs.reserve(its.size() * 4);
    items.reserve(its.size() * 2);
    for (size_t i = 0; i < its.size(); ++i) {
        if (i == 0 || its[i].tile != its[i - 1].tile || its[i].q != its[i - 1].q) {
            const uint32_t row[4] = {its[i].q, its[i].tile, (uint32_t)i, 0u};
            pairs.insert(pairs.end(), row, row + 4);
        }
        ++pairs[pairs.size() - 1];
        items.push_back(its[i].slot);
        items.push_back(its[i].local);
    }
}

// ------------------------------------------------------------------------------------------------ msr_rank_docs
constexpr uint32_t kRankNoSelf = 0xFFFFFFFFu;  // self[q] of a query without a self doc

struct RankPlan {
    std::vector<uint32_t> t_ptr;    // [nq + 1] the caller's, in 32 bits
    std::vector<uint32_t> e_query;  // [n_entries] query of each entry
    std::vector<uint32_t> self;     // [nq] ordinal that does not count for query q, or kRankNoSelf
    std::vector<uint32_t> pairs;    // [][4] {query, tile, first item, items (<= 65)}, tile-major
    std::vector<uint32_t> items;    // [][2] {slot in the scores, doc - doc0}: every listed doc (duplicates too) and self doc
};

inline void rank_plan(uint32_t tile, int nq, const int64_t* t_ptr, const uint32_t* t_ord, const int32_t* self_ord, RankPlan& pl) {
    const uint32_t n_ent = (uint32_t)t_ptr[nq];
    std::vector<ListedItem> its;
    its.reserve((size_t)n_ent + (size_t)nq);
    pl.t_ptr.assign(t_ptr, t_ptr + nq + 1);
    pl.e_query.resize(n_ent);
    pl.self.assign((size_t)nq, kRankNoSelf);
    for (int i = 0; i < nq; ++i) {
        for (int64_t e = t_ptr[i]; e < t_ptr[i + 1]; ++e) {
            its.push_back({t_ord[e] / tile, (uint32_t)i, (uint32_t)e, t_ord[e] % tile});
            pl.e_query[(size_t)e] = (uint32_t)i;
        }
        if (self_ord && self_ord[i] >= 0) {
            pl.self[(size_t)i] = (uint32_t)self_ord[i];
            its.push_back({(uint32_t)self_ord[i] / tile, (uint32_t)i, n_ent + (uint32_t)i, (uint32_t)self_ord[i] % tile});
        }
    }
    group_pairs(its, pl.pairs, pl.items);
}

// ------------------------------------------------------------------------------------------------ msr_explain_docs
constexpr uint32_t kExplainDense = 0x80000000u;  // ents[].x: dense-head slot in the low bits instead of a term id

struct ExplainPlan {
    std::vector<uint32_t> q_range;  // [nq][2] counting entries of query q = ents[x .. y)
    std::vector<uint32_t> ents;     // [][2] {term id | kExplainDense + dense slot, slot of the entry inside a row}
    std::vector<uint32_t> pairs;    // [][4] {query, tile, first item, items (<= 64)}, tile-major
    std::vector<uint32_t> items;    // [][2] {first output slot of the doc's row, doc - doc0}: the distinct docs of each pair
    std::vector<uint32_t> x_off;    // [n_entries] first output slot of target entry e
    std::vector<std::pair<uint32_t, uint32_t>> dups;  // (entry, the earlier entry of its query that lists the same doc)
};

inline void explain_plan(const HostIndex& hx, const int64_t* q_ptr, const int32_t* q_term, const int32_t* q_w, int nq,
                         uint32_t flags, const int64_t* t_ptr, const uint32_t* t_ord, ExplainPlan& pl) {
    const IndexHeader* h = hx.h;
    const uint32_t tile = h->tile_docs;
    // ---- the counting entries of every query that lists a doc
    std::vector<uint32_t>&qr = pl.q_range, &ents = pl.ents;
    qr.assign((size_t)nq * 2, 0u);
    for (int i = 0; i < nq; ++i) {
        if (t_ptr[i + 1] == t_ptr[i]) continue;
        qr[(size_t)i * 2] = (uint32_t)(ents.size() / 2);
        for (int64_t e = q_ptr[i]; e < q_ptr[i + 1]; ++e) {
            const int32_t t = q_term[e];
            if (t < 0 || q_w[e] <= 0) continue;
            if ((flags & MSR_F_DROP_DF_EQ_N) && hx.df[t] == h->n_docs) continue;
            if (hx.df[t] == 0) continue;  // no posting anywhere: every slot stays 0
            const int ds = hx.dense_slot[t];
            ents.push_back(ds >= 0 ? (kExplainDense | (uint32_t)ds) : (uint32_t)t);
            ents.push_back((uint32_t)(e - q_ptr[i]));
        }
        qr[(size_t)i * 2 + 1] = (uint32_t)(ents.size() / 2);
    }
    // ---- rows of the output; the distinct listed docs of each query (a repeated target is copied on the host after
    // the download); (query, tile) pairs, tile-major so that neighbouring workgroups share the tile
    pl.x_off.resize((size_t)t_ptr[nq]);
    std::vector<ListedItem> its;
    its.reserve((size_t)t_ptr[nq]);
    std::vector<std::pair<uint32_t, uint32_t>> srt;  // (ordinal, entry) of one query
    uint64_t at = 0;
    for (int i = 0; i < nq; ++i) {
        srt.clear();
        for (int64_t e = t_ptr[i]; e < t_ptr[i + 1]; ++e) {
            pl.x_off[(size_t)e] = (uint32_t)at;
            at += (uint64_t)(q_ptr[i + 1] - q_ptr[i]);
            srt.emplace_back(t_ord[e], (uint32_t)e);
        }
        if (qr[(size_t)i * 2] == qr[(size_t)i * 2 + 1]) continue;  // nothing counts: the rows stay 0
        std::sort(srt.begin(), srt.end());
        uint32_t first = 0;  // the lowest entry that lists the current ordinal
        for (size_t k = 0; k < srt.size(); ++k) {
            if (k > 0 && srt[k].first == srt[k - 1].first) {
                pl.dups.emplace_back(srt[k].second, first);
                continue;
            }
            first = srt[k].second;
            its.push_back({srt[k].first / tile, (uint32_t)i, pl.x_off[srt[k].second], srt[k].first % tile});
        }
    }
    group_pairs(its, pl.pairs, pl.items);
}

// ------------------------------------------------------------------------------------------------ msr_doc_vectors
constexpr uint32_t kDocvecStripeVecs = 8192;  // vecs (128 KiB of postings) one workgroup of docvec_tiles streams
constexpr uint32_t kDocvecSortRow = 2048;     // longest row docvec_order sorts on chip; longer rows are placed by counting

struct DocvecPlan {
    std::vector<uint32_t> ords;    // [rows] the distinct listed ordinals, ascending: row r of the device output
    std::vector<uint32_t> row_of;  // [n] row of listed entry e
    std::vector<uint32_t> work;    // [][4] {tile, first row, rows, stripe of the tile's vec range}, tile-major
};

// seg_ptr: the index's [n_tiles][n_terms + 1] table (absolute vec indexes); every ordinal is below n_docs.
inline void docvec_plan(const uint32_t* seg_ptr, uint32_t n_terms, uint32_t tile, const uint32_t* t_ord, int64_t n,
                        DocvecPlan& pl) {
    pl.ords.assign(t_ord, t_ord + n);
    std::sort(pl.ords.begin(), pl.ords.end());
    pl.ords.erase(std::unique(pl.ords.begin(), pl.ords.end()), pl.ords.end());
    pl.row_of.resize((size_t)n);
    for (int64_t e = 0; e < n; ++e)
        pl.row_of[(size_t)e] = (uint32_t)(std::lower_bound(pl.ords.begin(), pl.ords.end(), t_ord[e]) - pl.ords.begin());
    const size_t rows = pl.ords.size();
    for (size_t r0 = 0; r0 < rows;) {
        const uint32_t t = pl.ords[r0] / tile;
        size_t r1 = r0 + 1;
        while (r1 < rows && pl.ords[r1] / tile == t) ++r1;
        const uint32_t* sp = seg_ptr + (uint64_t)t * ((uint64_t)n_terms + 1);
        const uint32_t vecs = sp[n_terms] - sp[0];  // a tile without a vec (dense head only) gets no stripe
        for (uint32_t s = 0; (uint64_t)s * kDocvecStripeVecs < vecs; ++s) {
            const uint32_t row[4] = {t, (uint32_t)r0, (uint32_t)(r1 - r0), s};
            pl.work.insert(pl.work.end(), row, row + 4);
        }
        r0 = r1;
    }
}

}  // namespace msr
