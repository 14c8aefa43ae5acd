// Host side of msr_explain_docs (plain C++, no HIP; included by msr_explain.hpp): the tables explain_tiles reads, built
// from the caller's CSR arrays after the argument checks and the search path's query normalisation have passed (every
// term id of a counting entry is below n_terms, every ordinal below n_docs, at most MSR_EXPLAIN_MAX_TARGETS listed docs
// per query, fewer than 2^32 output slots).
#pragma once

#include <algorithm>
#include <utility>

#include "msr_internal.h"

namespace msr {

constexpr uint32_t kExplainDense = 0x80000000u;  // ents[].x: dense-head slot in the low bits instead of a term id

struct ExplainPlan {
    struct Item {
        uint32_t tile, q, row, local;  // row = first output slot of the listed doc, local = ordinal - tile * tile_docs
    };
    std::vector<uint32_t> q_range;  // [nq][2] counting entries of query q = ents[x .. y)
    std::vector<uint32_t> ents;     // [][2] {term id | kExplainDense + dense slot, slot of the entry inside a row}
    std::vector<uint32_t> pairs;    // [][4] {query, tile, first item, items (<= 64)}, tile-major
    std::vector<Item> items;        // the distinct listed docs of each pair
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
    std::vector<ExplainPlan::Item>& its = pl.items;
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
    std::stable_sort(its.begin(), its.end(), [](const ExplainPlan::Item& x, const ExplainPlan::Item& y) {
        return x.tile != y.tile ? x.tile < y.tile : x.q < y.q;
    });
    pl.pairs.reserve(its.size() * 4);
    for (size_t i = 0; i < its.size(); ++i) {
        if (i == 0 || its[i].tile != its[i - 1].tile || its[i].q != its[i - 1].q) {
            const uint32_t row[4] = {its[i].q, its[i].tile, (uint32_t)i, 0u};
            pl.pairs.insert(pl.pairs.end(), row, row + 4);
        }
        ++pl.pairs[pl.pairs.size() - 1];
    }
}

}  // namespace msr
