// Shared by the HIP translation units (msr_device.hip, msr_hybrid.hip, msr_filter.hip): device-side state of an index, kernel
// argument blocks, the resident query batch, and the few host functions that cross the unit boundary.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "msr_internal.h"

namespace msr {

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return MSR_E_HIP;                                                                  \
        }                                                                                      \
    } while (0)

// ------------------------------------------------------------------------------------------------ constants
constexpr int kQtBlock = 256;    // query terms staged in LDS per round
constexpr int kCandCap = 1024;   // candidate keys per workgroup (>= MSR_KMAX)
constexpr uint32_t kMaxGridY = 65535;  // HIP grid limit in y (tiles per launch)
constexpr uint64_t kMinStagedPairs = 4096;  // ... and only launches with at least this many (tile, query) pairs are staged
constexpr uint32_t kStage1Fraction = 16;  // staged search: 1/16 of the tiles (at least one) set the thresholds
constexpr size_t kZeroCopyBytes = 64u << 10;  // query block / result block of a small call (mapped host memory)
constexpr uint32_t kSmallMaxPairs = 1024;     // a small call launches at most this many (tile, query) workgroups
constexpr int kChunkVecs = 64;   // one chunk = one wave-wide uint4 load = 256 postings = 1 KiB
static_assert(kCandCap >= MSR_KMAX, "candidate buffer must hold k keys");
// score_tiles_walk (msr_walk.hpp): one workgroup per query walks the handle's tiles. Taken by light batches on handles
// of 2 .. kWalkMaxTiles tiles (more tiles than that no longer share the L2 between the workgroups in flight, which are
// spread over all of them), for k <= kWalkMaxK (the running top-k is one wave's worth of keys) and at least
// kWalkMinQueries queries (one round of resident workgroups: below it, tiles side by side finish a call sooner).
constexpr uint32_t kWalkMaxTiles = 8;
constexpr uint32_t kWalkMaxK = 64;
constexpr uint32_t kWalkMinQueries = 1024;
constexpr uint32_t kWalkRoundsMask = 7;  // WalkTile::doc0_rounds: doc0 is a multiple of the tile size, rounds <= 4

// ------------------------------------------------------------------------------------------------ tile shapes
// The launch shape of every kernel that works on one doc tile: <tile, threads, chunk loads per bank, min waves/SIMD of
// the k <= 512 instance, of the other instances>. `light` marks the small tiles: only they have a light scorer
// (score_tiles<..., LIGHT>) and the hybrid kernels (hybrid_tiles, fuse_tiles).
template <uint32_t DOCS, uint32_t THREADS, uint32_t LOADS, uint32_t WAVES, uint32_t WAVES_REST>
struct TileShape {
    static constexpr uint32_t docs = DOCS, threads = THREADS, loads = LOADS, waves = WAVES, waves_rest = WAVES_REST;
    static constexpr bool light = DOCS == 4096 || DOCS == 8192;
};

// Calls f(TileShape<...>{}) for the shape of `tile_docs`; false: no such shape. THE table: every launcher goes through it.
template <class F>
inline bool with_tile_shape(uint32_t tile_docs, F&& f) {
    // LDS per workgroup = 4 B x tile + 4-8 KiB candidates + maxima -> workgroups (waves) per CU:
    switch (tile_docs) {
        case 32768: f(TileShape<32768, 1024, 8, 4, 4>{}); return true;  // 1 (16)
        case 16384: f(TileShape<16384, 512, 8, 4, 4>{}); return true;   // 2 (16)
        case 12288: f(TileShape<12288, 512, 4, 4, 4>{}); return true;   // 2 (16)
        case 8192: f(TileShape<8192, 512, 4, 8, 6>{}); return true;     // 4 (32) with k <= 512, 3 (24) above
        case 4096: f(TileShape<4096, 256, 4, 6, 5>{}); return true;     // 7 (28)
        default: return false;
    }
}

// device_attach refuses an index whose tile size has no shape, so the launchers never get here with an open handle
inline int no_tile_shape(uint32_t tile_docs) {
    set_error("no kernel instance for tile_docs=%u (supported: 4096, 8192, 12288, 16384, 32768)", tile_docs);
    return MSR_E_RANGE;
}

inline uint32_t tile_threads(uint32_t tile_docs) {  // of the tile's scoring and selection instances (0: no such shape)
    uint32_t n = 0;
    with_tile_shape(tile_docs, [&](auto s) { n = s.threads; });
    return n;
}

inline bool hybrid_tile(uint32_t tile_docs) {  // the tile sizes the hybrid kernels are instantiated for
    bool yes = false;
    with_tile_shape(tile_docs, [&](auto s) { yes = s.light; });
    return yes;
}

// One tile as score_tiles_walk sees it: what score_tiles computes per workgroup from ScoreArgs, built once per handle
// (fill_walk_tiles) because it depends on the index alone. 32 bytes: one scalar load per tile.
struct WalkTile {
    const uint32_t* seg_row;  // the tile's row of seg_ptr
    const char* post_base;    // address of the tile's first posting vec
    const char* dense;        // the tile's dense-head rows
    uint32_t tile_first;      // seg_row[0]
    uint32_t doc0_rounds;     // first doc ordinal of the tile | rounds of 4*NT accumulators that hold real docs
};
static_assert(sizeof(WalkTile) == 32, "one s_load_dwordx8 per tile");

// Caching device allocator of one index handle. msr_search_csr at the reference's call shape (4 queries per call,
// scripts/search_sparse.sh:16) would otherwise spend more time in hipMalloc / hipFree than in its kernels.
struct DevicePool {
    static constexpr size_t kMaxCachedBlock = 64ull << 20, kMaxCachedTotal = 512ull << 20;
    std::vector<std::pair<size_t, void*>> free_;  // (bytes, ptr)
    size_t cached = 0;
    static size_t round_up(size_t b) {
        size_t r = 256;
        while (r < b) r <<= 1;
        return r;
    }
    void* alloc(size_t bytes) {
        const size_t want = round_up(std::max<size_t>(bytes, 1));
        for (size_t i = 0; i < free_.size(); ++i)
            if (free_[i].first == want) {
                void* p = free_[i].second;
                free_[i] = free_.back();
                free_.pop_back();
                cached -= want;
                return p;
            }
        void* p = nullptr;
        if (hipMalloc(&p, want) != hipSuccess) return nullptr;
        return p;
    }
    void release(void* p, size_t bytes) {
        if (!p) return;
        const size_t have = round_up(std::max<size_t>(bytes, 1));
        if (have > kMaxCachedBlock || cached + have > kMaxCachedTotal) {
            (void)hipFree(p);
            return;
        }
        free_.emplace_back(have, p);
        cached += have;
    }
    void purge() {
        for (auto& e : free_) (void)hipFree(e.second);
        free_.clear();
        cached = 0;
    }
};

struct DeviceIndex {
    int device = -1;
    hipStream_t stream = nullptr;
    DevicePool pool;
    std::vector<hipEvent_t> spare_events;  // recycled by the calls on this handle: borrow_event / return_event only
    void* h_stage = nullptr;               // pinned staging for small uploads / downloads
    size_t h_stage_bytes = 0;
    hipEvent_t stage_ev = nullptr;         // recorded after an async upload out of h_stage ...
    bool stage_pending = false;            // ... and waited for before the buffer is written or freed again
    // small calls (the reference's 4 queries per batch_search): the kernels read the queries from, and write the results
    // to, mapped pinned host memory — no upload and no download on the stream (each costs it ~3.5 us, scripts/latency_lab.hip)
    void* h_zc = nullptr;                  // hipHostMalloc(mapped), 2 x kZeroCopyBytes: queries | results
    void* d_zc = nullptr;                  // its device view
    uint32_t* d_seg_ptr = nullptr;   // [shard_ntiles][n_terms+1] absolute vec index
    uint32_t* d_postings = nullptr;  // the shard's vecs; vec v of the index lives at d_postings + (v - vec_base)*4
    uint32_t* d_dense = nullptr;     // [shard_ntiles][n_pairs][tile_docs] dense head of the shard's tiles
    uint32_t n_pairs = 0;            // dense-head pairs resident per tile (all of them, or those with an owned term)
    std::vector<int32_t> pair_local; // index pair p -> resident pair (or -1); identity unless the handle is a term shard
    uint32_t seg_terms = 0;          // terms per row of d_seg_ptr (n_terms, or term_hi - term_lo on a term shard)
    uint32_t term_base = 0;          // query term ids are rebased by this before upload (term_lo on a term shard)
    WalkTile* d_walk = nullptr;       // [shard_ntiles] tile side of score_tiles_walk, or null: the handle never walks
    uint64_t resident_bytes = 0;     // d_seg_ptr + d_postings + d_dense
    uint32_t vec_base = 0;
    uint64_t shard_vecs = 0;
    std::vector<uint32_t> df_shard;  // postings of each term inside this shard (for algorithmic bytes)
    bool df_shard_ready = false;
    // exchange
    ncclComm_t comm = nullptr;
    int n_ranks = 1;
    int rank = 0;

    // a timing event: a spare one, else a new one (null: hipEventCreate failed); handed back, at most 64 are kept
    hipEvent_t borrow_event() {
        hipEvent_t e = nullptr;
        if (!spare_events.empty()) {
            e = spare_events.back();
            spare_events.pop_back();
        } else if (hipEventCreate(&e) != hipSuccess) {
            e = nullptr;
        }
        return e;
    }
    void return_event(hipEvent_t e) {
        if (!e) return;
        if (spare_events.size() < 64)
            spare_events.push_back(e);
        else
            (void)hipEventDestroy(e);
    }
};

// false, with the error set to "<who>: <what> failed: <HIP's words>", unless e is hipSuccess
inline bool hip_ok(const char* who, hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    set_error("%s: %s failed: %s", who, what, hipGetErrorString(e));
    return false;
}

// ------------------------------------------------------------------------------------------------ kernel arguments
struct ScoreArgs {
    const uint32_t* seg_ptr;   // [ntiles][n_terms+1]
    const uint32_t* postings;  // shard base
    const uint4* q_meta;       // [nq] {first term, end term, bit mask of the query's dense-head pairs, 0}
    const uint32_t* q_term;
    const uint32_t* q_w;
    const uint32_t* dense;     // [ntiles][n_pairs][TILE_DOCS] dense head (weights of term 2p+1 << 16 | term 2p)
    const uint32_t* q_dense;   // [nq][n_pairs] packed query weights of the dense-head terms (0 = absent)
    uint32_t n_pairs;
    uint64_t* part;            // [ntiles][nq][k] keys
    const uint64_t* theta;     // [nq][k] best keys of an earlier launch's tiles (staged search), or null
    uint32_t unsorted;         // 1: the tile's k keys may be emitted in any order (single-tile hybrid lists)
    uint64_t n_docs;           // whole index
    uint32_t vec_base;
    uint32_t n_terms;
    uint32_t tile0;            // first (global) tile of the shard
    uint32_t tl0;              // first shard-local tile of this launch (grid y is limited to 65535 tiles)
    uint32_t nq;               // queries of the batch (row stride of `part`)
    uint32_t q0;               // this launch scores queries [q0, q0 + qn)
    uint32_t qn;
    uint32_t k;
    // term-sharded search (MODE 1): instead of selecting, the accumulator tile is written (or added) to
    // dump[((g * qn + (q - q0)) * tpr + t) * TILE_DOCS + i] with g = tile / tpr, t = tile % tpr  — the layout whose
    // G equal chunks are the doc ranges that ncclReduceScatter hands to the G ranks
    uint32_t* dump;
    uint32_t tpr;              // tiles per rank = ceil(n_tiles / G)
    uint32_t dump_add;         // 1: dump[...] += tile (single-GPU emulation of the reduction), 0: store
    uint32_t light;            // 1: every query of the batch holds <= 64 sparse terms (score_tiles<..., LIGHT>)
};

struct SelectArgs {
    const uint32_t* src;
    uint64_t* part;   // [tpr][nq][k]
    uint64_t n_docs;
    uint32_t n_tiles; // tiles of the whole index
    uint32_t tpr;
    uint32_t rank;
    uint32_t nq, q0, qn, k;
    uint32_t unsorted;  // as ScoreArgs::unsorted
};

struct MergeArgs {
    const uint64_t* lists;   // key(list, q, j) = lists[list*list_stride + q*k + j]; 0 = empty slot
    uint64_t list_stride;
    uint32_t n_lists;
    uint32_t nq;
    uint32_t k;
    uint64_t* out_keys;      // [nq][k] (may be null)
    uint32_t* out_ord;       // [nq][k] (may be null)
    uint32_t* out_score_u32;
    float* out_score;
    int32_t* out_n;
};

struct WalkArgs {
    ScoreArgs s;            // the query side and n_pairs (the tile side comes from `tiles`)
    MergeArgs m;            // the result rows (lists / list_stride / n_lists unused)
    const WalkTile* tiles;  // [n_tiles]
    uint32_t n_tiles;
};

// The routing rule of batch_search_local: does a search of `nq` queries at depth k take score_tiles_walk? `has_table`:
// the handle holds a WalkTile table (2 .. kWalkMaxTiles tiles of 4096 or 8192 docs, every term resident).
inline bool walk_route(bool has_table, bool light_batch, bool list_as_set, uint32_t nq, uint32_t k) {
    return has_table && light_batch && !list_as_set && k <= kWalkMaxK && nq >= kWalkMinQueries;
}

// deep_select_rows (msr_deep_select.hpp): exact top-k, k <= MSR_DEEP_KMAX, of rows of u32 keys that sit in HBM
struct DeepArgs {
    const uint32_t* src;  // key(row, col) = src[row * ld + col], valid columns [0, n); key 0 = not a member
    uint64_t ld;          // a multiple of 4, src 16-byte aligned
    uint32_t n;
    uint32_t rows;
    uint32_t k;
    uint32_t* out_idx;    // [rows][k] columns of the k best members by (key desc, col asc); 0xFFFFFFFF past out_n
    uint32_t* out_key;    // [rows][k] their keys; 0 past out_n
    float* out_f32;       // [rows][k] (float)key, or null
    int32_t* out_n;       // [rows] min(k, members)
};

// Filtered search (msr_filter.hpp): the doc sets of one call as the kernels read them.
struct FilterArgs {
    const uint32_t* bits;  // [n_sets][stride]: bit (o & 31) of word (o >> 5) of row s = doc / row o belongs to set s
    const uint8_t* any;    // [n_sets][n_tiles]: does set s hold a doc of tile t
    const int32_t* q_set;  // [nq of the call]: the set of each query, -1 = unfiltered
    uint32_t stride;       // words per bitmap row = n_tiles * tile_docs / 32 (zero padded: a ragged last tile reads in bounds)
    uint32_t n_tiles;      // tiles of the whole index
};

// The host image of a call's doc sets, shared by msr_search_filtered and msr_dense_search_filtered. `set_bits` is the
// caller's [n_sets][(n + 31) / 32] bitmap over n docs / rows, `q_set` its per-query choice (may be null: no set -> every
// query unfiltered, one set -> every query uses it). One pass copies every row into the device layout (row stride
// n_tiles * tile_docs / 32 words, zero padded), clears the bits at or above n and fills any[set][tile].
struct FilterImage {
    std::vector<uint32_t> bits;   // [n_sets][stride]
    std::vector<uint32_t> any;    // n_sets * n_tiles bytes, packed into words for the upload
    std::vector<uint32_t> q_set;  // [nq] (int32 values)
    uint32_t stride = 0;
    void build(const uint32_t* set_bits, int n_sets, const int32_t* q_set_in, int nq, uint64_t n, uint32_t tile_docs,
               uint32_t n_tiles) {
        const uint64_t w_in = (n + 31) / 32;
        const uint32_t tile_words = tile_docs / 32;
        stride = n_tiles * tile_words;
        bits.assign(std::max<size_t>((size_t)n_sets * stride, 1), 0u);
        any.assign(((size_t)n_sets * n_tiles + 3) / 4 + 1, 0u);
        uint8_t* const any8 = reinterpret_cast<uint8_t*>(any.data());
        for (int s = 0; s < n_sets; ++s) {
            uint32_t* row = bits.data() + (size_t)s * stride;
            if (w_in) memcpy(row, set_bits + (size_t)s * w_in, (size_t)w_in * 4);
            if (n % 32) row[w_in - 1] &= (1u << (n % 32)) - 1u;  // bits at or above n cannot surface a padding doc
            for (uint32_t t = 0; t < n_tiles; ++t) {
                uint32_t acc = 0;
                for (uint32_t w = 0; w < tile_words; ++w) acc |= row[(size_t)t * tile_words + w];
                any8[(size_t)s * n_tiles + t] = acc != 0;
            }
        }
        q_set.resize(std::max(nq, 1));
        for (int i = 0; i < nq; ++i) q_set[i] = (uint32_t)(q_set_in ? q_set_in[i] : (n_sets == 0 ? -1 : 0));
    }
};

// The argument checks of the two filtered calls that concern the sets. Shapes (MSR_E_INVAL) ...
inline int filter_check_shapes(const char* who, const uint32_t* set_bits, int n_sets, const int32_t* q_set) {
    if (n_sets < 0 || (n_sets > 0 && !set_bits) || (n_sets > 1 && !q_set)) {
        set_error("%s: bad doc sets (n_sets = %d%s%s)", who, n_sets, n_sets > 0 && !set_bits ? ", null set_bits" : "",
                  n_sets > 1 && !q_set ? ", null q_set with more than one set" : "");
        return MSR_E_INVAL;
    }
    return MSR_OK;
}
// ... and ranges (MSR_E_RANGE).
inline int filter_check_ranges(const char* who, int n_sets, const int32_t* q_set, int nq) {
    if (n_sets > MSR_FILTER_MAX_SETS) {
        set_error("%s: %d doc sets, at most MSR_FILTER_MAX_SETS = %d", who, n_sets, MSR_FILTER_MAX_SETS);
        return MSR_E_RANGE;
    }
    for (int i = 0; q_set && i < nq; ++i)
        if (q_set[i] < -1 || q_set[i] >= n_sets) {
            set_error("%s: q_set[%d] = %d is outside [-1, n_sets = %d)", who, i, q_set[i], n_sets);
            return MSR_E_RANGE;
        }
    return MSR_OK;
}

// The refusal of the calls that read the whole index (listed docs, deep and filtered search, doc vectors) on a shard handle
inline int whole_index_check(const char* who, const msr_index* ix) {
    if (ix->term_nshards > 0 || ix->shard_ntiles != ix->host.h->n_tiles) {
        set_error("%s: the call needs every doc and every term of the index; this handle is a %s shard (open the whole "
                  "index with msr_index_open)", who, ix->term_nshards > 0 ? "term-range" : "doc-range");
        return MSR_E_INVAL;
    }
    return MSR_OK;
}

// ... and of every device call on a handle opened without a device; `missing` names the CPU path there is none of
inline int device_check(const msr_index* ix, const char* missing = "scoring path") {
    if (!ix->dev) {
        set_error("index handle has no HIP device bound (opened with device < 0); there is no CPU %s", missing);
        return MSR_E_NODEVICE;
    }
    return MSR_OK;
}

// defined in msr_device.hip
int launch_select(hipStream_t st, uint32_t tile_docs, const SelectArgs& a);
int launch_merge(hipStream_t st, const MergeArgs& a);
int launch_deep_select(hipStream_t st, const DeepArgs& a);
int launch_score_dump(hipStream_t st, uint32_t tile_docs, uint32_t n_tiles, const ScoreArgs& a);  // score_tiles<dump>, every tile
// defined in msr_filter.hip
int launch_score_filtered(hipStream_t st, uint32_t tile_docs, uint32_t t_begin, uint32_t t_end, const ScoreArgs& a0,
                          const FilterArgs& f);
int launch_select_filtered(hipStream_t st, uint32_t tile_docs, const SelectArgs& a, const FilterArgs& f);
int launch_score_dump_filtered(hipStream_t st, uint32_t tile_docs, uint32_t n_tiles, const ScoreArgs& a0, const FilterArgs& f);
int launch_mask_key_rows(hipStream_t st, uint32_t* D, uint64_t ld, uint32_t rows, uint32_t q0, const FilterArgs& f);

}  // namespace msr

struct msr_batch {
    msr_index* ix = nullptr;
    bool unsorted_ok = false;  // hybrid path: the consumer of d_keys treats each query's list as a set
    bool zero_copy = false;    // small call: d_qptr .. d_qdense and d_ord .. d_n are device views of the handle's mapped host block
    bool untimed = false;      // no HIP events around the kernels (msr_search_csr's own batches)
    int nq = 0;
    int kmax = 0;
    int last_k = 0;
    uint64_t nnz = 0;             // kept query entries
    uint64_t sum_df = 0;          // sum over kept entries of df_shard(term)
    uint64_t sum_df_dense = 0;    // ... of which the dense-head terms' (scored doc-major, no inverted list)
    uint32_t max_sparse_terms = 0; // most sparse (non dense-head) terms in one query: <= 64 selects the light kernel
    uint32_t* d_qptr = nullptr;
    uint32_t* d_qterm = nullptr;
    uint32_t* d_qw = nullptr;
    uint32_t* d_qdense = nullptr; // [nq][n_pairs]
    uint64_t* d_part = nullptr;   // [ntiles][nq][kmax]
    uint64_t* d_keys = nullptr;   // [nq][kmax] local top-k keys
    uint64_t* d_gather = nullptr; // [n_ranks][nq][kmax] (sharded search)
    uint32_t* d_ord = nullptr;
    uint32_t* d_su32 = nullptr;
    float* d_sf32 = nullptr;
    int32_t* d_n = nullptr;
    // term-sharded search
    uint32_t* d_S = nullptr;      // [G][Qt][tpr*tile] partial accumulators of one query tile (reduce-scatter send buffer)
    uint32_t* d_R = nullptr;      // [Qt][tpr*tile] summed accumulators of this rank's doc range
    uint64_t* d_tpart = nullptr;  // [tpr][nq][kmax] per-tile keys of this rank's doc range
    size_t S_elems = 0, R_elems = 0, tpart_elems = 0;
    int term_shard = -1, term_nshards = 0;  // >= 0: the batch holds only the query terms of that term range
    std::vector<std::pair<void*, size_t>> pooled;  // blocks taken from the index's DevicePool (the d_* above point into them)
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;  // the current call's events (borrowed from `events`)
    std::vector<hipEvent_t> events;  // 3 per recorded search call since the last timing reset
    size_t calls = 0;                // recorded calls
    uint64_t walks = 0;              // searches of this batch that took score_tiles_walk (msr_batch_debug_stamps)
    bool timed = false;
};

// defined in msr_device.hip
void batch_free(msr_batch* b);          // release + unregister from the index + delete
void batch_release_device(msr_batch* b); // device buffers and events only (the index is being closed)
extern "C" int batch_search_local(msr_batch* b, int k, bool final_arrays);  // internal, not part of include/msr.h
void fill_score_args(msr::ScoreArgs& sa, msr_batch* b, int k);  // a launch over the whole batch and every tile

// The device scratch of one call on a handle: the pool blocks it handed out, the events it borrowed and (optionally) the
// call's batch. Leaving the scope waits for the stream unless the call set `ok` (nothing in flight may still use the
// scratch), then gives the blocks back to the pool, the events back to the handle and frees the batch, in this order.
struct CallScratch {
    const char* who;  // the call, as its error messages name it
    msr::DeviceIndex* d;
    msr_batch* b;
    bool ok = false;  // the call succeeded: its last step waited for the stream already
    std::vector<std::pair<void*, size_t>> blocks;
    std::vector<hipEvent_t> events;  // the call's laps, when it is timed
    bool timed = false;
    CallScratch(const char* name, msr::DeviceIndex* dev, msr_batch* batch = nullptr) : who(name), d(dev), b(batch) {}
    CallScratch(const CallScratch&) = delete;
    CallScratch& operator=(const CallScratch&) = delete;
    ~CallScratch() {
        if (!ok) (void)hipStreamSynchronize(d->stream);
        for (auto& blk : blocks) d->pool.release(blk.first, blk.second);
        for (hipEvent_t e : events) d->return_event(e);
        batch_free(b);
    }
    std::vector<uint32_t> in;  // the call's upload block: u32 sub-buffers, each starting on a 256-byte boundary
    size_t put(const uint32_t* src, size_t n) {  // appends a sub-buffer of n words; its first word
        const size_t at = in.size();
        in.resize(at + (n + 63) / 64 * 64, 0u);
        if (n) memcpy(in.data() + at, src, n * 4);
        return at;
    }
    size_t put(const std::vector<uint32_t>& v) { return put(v.data(), v.size()); }
    uint32_t* alloc(size_t bytes) {  // null: out of device memory
        void* p = d->pool.alloc(bytes);
        if (p) blocks.emplace_back(p, bytes);
        return (uint32_t*)p;
    }
    // The block built with put(), copied to the device (`what` names its content in the messages). Null: *rc and the
    // error are set.
    uint32_t* upload(const char* what, int* rc) {
        const size_t bytes = in.size() * 4;
        uint32_t* p = alloc(bytes);
        if (!p) {
            msr::set_error("%s: device allocation failed (%zu bytes of %s)", who, bytes, what);
            *rc = MSR_E_NOMEM;
            return nullptr;
        }
        const hipError_t e = hipMemcpy(p, in.data(), bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) return p;
        msr::set_error("%s: upload of the %s failed: %s", who, what, hipGetErrorString(e));
        *rc = MSR_E_HIP;
        return nullptr;
    }
    // The call's timing laps: laps(n, want) borrows n events when the caller asked for times, mark(i) records event i on
    // the stream, elapsed(i, j, out) reads the milliseconds from mark i to mark j. An untimed call does nothing in the
    // last two. Each returns the call's error code.
    int laps(int n, bool want) {
        timed = want;
        for (int i = 0; timed && i < n; ++i) {
            hipEvent_t e = d->borrow_event();
            if (!e) {
                msr::set_error("%s: hipEventCreate failed", who);
                return MSR_E_HIP;
            }
            events.push_back(e);
        }
        return MSR_OK;
    }
    int mark(int i) {
        return !timed || msr::hip_ok(who, hipEventRecord(events[i], d->stream), "hipEventRecord") ? MSR_OK : MSR_E_HIP;
    }
    int elapsed(int i, int j, float* out) {
        return !timed || msr::hip_ok(who, hipEventElapsedTime(out, events[i], events[j]), "hipEventElapsedTime") ? MSR_OK : MSR_E_HIP;
    }
};
